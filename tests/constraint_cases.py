"""Case table and plain-Python reference of constrained decoding (aki_amd/constraint.py; the mask stage of process_row and the state store
of pick_finish in aki_amd/csrc/decode.hip).

numpy only.  tests/test_constraint_cases_cpu.py checks the builders and the reference itself (against the installed transformers'
PrefixConstrainedLogitsProcessor); tests/test_constraint_gpu.py runs the cases on the device.

The reference works on the table `TokenConstraint.with_eos(eos)` returns - int32 [S, V], -1 = not allowed:
  mask(table, s)            bool [V]: the tokens state s allows
  walk(table, start, toks)  the states a token row passes through, [len(toks) + 1]; -1 from the first token that is not allowed
  greedy(table, start, scores, eos)  per step: the allowed token with the largest score (lowest index among equals), the next state;
                            after an eos the row is finished: pad, state kept
"""
from dataclasses import dataclass
from typing import Tuple

import numpy as np


@dataclass
class Case:
    name: str
    V: int
    choices: Tuple[Tuple[int, ...], ...]
    eos: Tuple[int, ...]


CASES = [
    Case("abcd", 64, ((5,), (6,), (7,), (8,)), (2,)),
    Case("prefix-of-another", 64, ((5, 6), (5, 6, 7), (9,)), (2,)),
    Case("shared-prefix", 1003, ((10, 11, 12), (10, 11, 13), (10, 20), (1002,)), (0, 1)),
    Case("duplicates", 64, ((3, 4), (3, 4), (4, 3)), (63,)),
    Case("wide", 32067, ((32066, 1), (32066, 32065, 7), (8, 8, 8, 8)), (32000, 32007)),
]


def mask(table: np.ndarray, s: int) -> np.ndarray:
    return table[s] >= 0


def walk(table: np.ndarray, start: int, toks) -> list:
    out, s = [int(start)], int(start)
    for t in toks:
        s = int(table[s, int(t)]) if s >= 0 else -1
        out.append(s)
    return out


def legal(table: np.ndarray, start: int, toks) -> bool:
    return min(walk(table, start, toks)) >= 0


def greedy(table: np.ndarray, start: int, scores: np.ndarray, eos, pad: int):
    """scores [steps, V] -> (tokens [steps], states [steps + 1], done_at or -1)."""
    toks, states, s, done_at = [], [int(start)], int(start), -1
    for t in range(scores.shape[0]):
        if done_at >= 0:
            toks.append(pad)
            states.append(s)
            continue
        x = np.where(mask(table, s), scores[t].astype(np.float64), -np.inf)
        tok = int(np.argmax(x))                    # the first of equal maxima, as the pick
        toks.append(tok)
        s = int(table[s, tok])
        states.append(s)
        if tok in eos:
            done_at = t
    return toks, states, done_at


def allowed_fn(table: np.ndarray, start: int):
    """HF's prefix_allowed_tokens_fn(batch_id, input_ids) for one automaton: the tokens allowed behind the generated prefix."""
    def fn(batch_id, input_ids):
        s = walk(table, start, [int(t) for t in input_ids])[-1]
        return np.flatnonzero(mask(table, s)).tolist()
    return fn


def histories(c: Case, table: np.ndarray, start: int):
    """Legal generated prefixes of length 0, 1 and 3 (the longest one possible where the case has no walk that long; an accepted choice is
    continued with eos, which loops)."""
    out = []
    for want in (0, 1, 3):
        best = []
        for ch in c.choices:
            h = (list(ch) + [c.eos[0]] * want)[:want]
            if legal(table, start, h) and len(h) >= len(best):
                best = h
        out.append(best)
    return out
