"""Constrained decoding for `generate(..., constraint=...)`: a deterministic finite automaton over token ids, built and checked on the host
and applied on the device (aki_amd/csrc/decode.hip: the last stage of process_row masks what the row's state forbids, pick_finish stores
the next state).  Pure host code: importing this module needs neither the HIP library nor a GPU; only `bind` touches torch.

An automaton is
    next_state  int array [S, V]: the state behind token v in state s, -1 where v is not allowed
    accepting   bool array [S]: the states in which the sequence may end (an eos id may be emitted)
    starts      one or more start states: one constraint has one, `union` gives one per member
`TokenConstraint.from_choices` builds the trie of a closed answer set; `from_table` is the seam for anything compiled elsewhere (a regular
expression, a JSON schema: such compilers are not part of this package).

`ConstraintPool` is the form `generate_many` takes: the constraints of a queue's requests as one device table, each keeping its own state
numbers, so the state limit holds per constraint and not per call.

Greedy decoding inside a trie follows the locally best allowed token: it does NOT return the most likely choice as a whole (a choice whose
first token is unlikely but whose rest is certain loses to one with a likely first token).  To rank a closed set of answers by their
likelihood use `AKI.score`, which scores every answer teacher-forced behind one prefill.
"""
from __future__ import annotations

from collections import deque
from typing import List, Optional, Sequence

import numpy as np

MAX_STATES = 32767                     # the device table is int16
DEFAULT_MAX_TABLE_BYTES = 256 << 20


class TokenConstraint:
    def __init__(self, next_state: np.ndarray, accepting: np.ndarray, starts: Sequence[int]):
        nxt = np.asarray(next_state)
        acc = np.asarray(accepting)
        if nxt.ndim != 2 or nxt.shape[0] < 1 or nxt.shape[1] < 1 or nxt.dtype.kind not in "iu":
            raise ValueError(f"next_state is an integer array [S, V] with S, V >= 1, got {nxt.dtype} {tuple(nxt.shape)}")
        S, V = nxt.shape
        if acc.shape != (S,) or acc.dtype.kind not in "biu":
            raise ValueError(f"accepting is a bool array [S] = [{S}], got {acc.dtype} {tuple(acc.shape)}")
        if S > MAX_STATES:
            raise ValueError(f"a token constraint holds at most {MAX_STATES} states, got {S}")
        nxt = nxt.astype(np.int32)
        if int(nxt.min()) < -1 or int(nxt.max()) >= S:
            raise ValueError(f"next_state entries are -1 (not allowed) or a state in [0, {S})")
        starts = [int(s) for s in starts]
        if not starts or any(not 0 <= s < S for s in starts):
            raise ValueError(f"every start state has to be in [0, {S}), got {starts}")
        self.next_state, self.accepting, self.starts = nxt, acc.astype(bool), starts
        self._with_eos = None           # the last with_eos result: (eos ids, table); next_state is not meant to be changed afterwards

    @property
    def n_states(self) -> int:
        return self.next_state.shape[0]

    @property
    def V(self) -> int:
        return self.next_state.shape[1]

    @classmethod
    def from_table(cls, next_state, accepting, start=0) -> "TokenConstraint":
        """An automaton compiled elsewhere: next_state [S, V] (-1 = not allowed), accepting [S], start: one state or a list of them."""
        return cls(next_state, accepting, [start] if isinstance(start, (int, np.integer)) else list(start))

    @classmethod
    def from_choices(cls, choices, V: int) -> "TokenConstraint":
        """The trie of a closed set of answers: `choices` is a non-empty list of non-empty token-id lists, V the logits' width.  A state
        accepts exactly where a choice ends; a choice may be a prefix of another; equal choices collapse."""
        V = int(V)
        if V < 1:
            raise ValueError(f"a vocabulary of {V} columns")
        choices = list(choices) if choices is not None else []
        if not choices:
            raise ValueError("from_choices takes a non-empty list of non-empty token-id lists")
        edges, accepting = [{}], [False]
        for ch in choices:
            if isinstance(ch, (int, np.integer)) or len(ch) == 0:
                raise ValueError("from_choices takes a non-empty list of non-empty token-id lists")
            s = 0
            for tok in ch:
                tok = int(tok)
                if not 0 <= tok < V:
                    raise ValueError(f"token id {tok} is outside [0, {V})")
                if tok not in edges[s]:
                    edges[s][tok] = len(edges)
                    edges.append({})
                    accepting.append(False)
                s = edges[s][tok]
            accepting[s] = True
        if len(edges) > MAX_STATES:
            raise ValueError(f"a token constraint holds at most {MAX_STATES} states, the trie has {len(edges)}")
        nxt = np.full((len(edges), V), -1, dtype=np.int32)
        for s, e in enumerate(edges):
            for tok, d in e.items():
                nxt[s, tok] = d
        return cls(nxt, np.asarray(accepting, dtype=bool), [0])

    @classmethod
    def union(cls, members: Sequence["TokenConstraint"]) -> "TokenConstraint":
        """One table for several constraints over the same V, the members' state numbers offset by the states in front of them: one start
        state per member's start state, in order - `generate(constraint=[c_0 .. c_{B-1}])` gives sample b the b-th."""
        members = list(members)
        if not members or any(not isinstance(m, TokenConstraint) for m in members):
            raise ValueError("union takes a non-empty list of TokenConstraint")
        V = members[0].V
        if any(m.V != V for m in members):
            raise ValueError(f"union: every member has to be built for the same V, got {[m.V for m in members]}")
        tables, starts, off = [], [], 0
        for m in members:
            tables.append(np.where(m.next_state >= 0, m.next_state + off, -1))
            starts += [s + off for s in m.starts]
            off += m.n_states
        return cls(np.concatenate(tables, axis=0), np.concatenate([m.accepting for m in members]), starts)

    def with_eos(self, eos_ids) -> np.ndarray:
        """The table `bind` puts on the device, as int32 [S, V]: for every eos id e, column e of state s is s itself (a self loop) where s
        accepts and -1 elsewhere.  An ordinary transition on an eos id, and a state that can be reached from a start state and allows
        nothing, raise ValueError: the kernel never meets a row with nothing allowed."""
        eos = sorted({int(e) for e in (eos_ids or [])})
        if any(not 0 <= e < self.V for e in eos):
            raise ValueError(f"every eos id has to be in [0, {self.V}), got {eos}")
        if self._with_eos is not None and self._with_eos[0] == eos:      # generate checks before the prefill and binds behind it
            return self._with_eos[1]
        nxt = self.next_state.copy()
        for e in eos:
            if bool((nxt[:, e] >= 0).any()):
                raise ValueError(f"eos id {e} is used as an ordinary transition of the constraint: it can only end an accepted sequence")
            nxt[:, e] = np.where(self.accepting, np.arange(self.n_states), -1)
        seen = np.zeros(self.n_states, dtype=bool)
        seen[self.starts] = True
        todo = deque(self.starts)
        while todo:
            s = todo.popleft()
            out = np.unique(nxt[s][nxt[s] >= 0])
            if out.size == 0:
                raise ValueError(f"state {s} can be reached and allows no token" + (" (it accepts, but there is no eos id to emit)"
                                                                                   if self.accepting[s] and not eos else ""))
            for d in out[~seen[out]]:
                seen[d] = True
                todo.append(int(d))
        self._with_eos = (eos, nxt)
        return nxt

    def bind(self, eos_ids, device, rows_start: Optional[Sequence[int]] = None,
             max_table_bytes: int = DEFAULT_MAX_TABLE_BYTES) -> "BoundConstraint":
        """The device form for one `generate` call: the table of `with_eos(eos_ids)` as int16 [S, V] on `device` (row stride padded to a
        multiple of 8, so that every row is 16-byte aligned), and the start state of every row, `rows_start` (default: the start states)."""
        S, V = self.next_state.shape
        if S > MAX_STATES:
            raise ValueError(f"a token constraint holds at most {MAX_STATES} states, got {S}")
        if S * V * 2 > int(max_table_bytes):
            raise ValueError(f"the constraint's device table needs {S} * {V} * 2 = {S * V * 2} bytes, above max_table_bytes = {int(max_table_bytes)}")
        rows = [int(s) for s in (self.starts if rows_start is None else rows_start)]
        if not rows or any(not 0 <= s < S for s in rows):
            raise ValueError(f"rows_start: every row's start state has to be in [0, {S})")
        nxt = self.with_eos(eos_ids)
        import torch
        ld = (V + 7) // 8 * 8
        table = torch.full((S, ld), -1, dtype=torch.int16, device=device)
        table[:, :V] = torch.from_numpy(nxt.astype(np.int16)).to(device)
        return BoundConstraint(table, V, S, torch.tensor(rows, dtype=torch.int32, device=device))


class BoundConstraint:
    """What ops.LogitsProcessors takes as `constraint`: table int16 [S, ld >= V] (a view of width V is `.table[:, :V]`), row_start int32
    [rows]."""

    def __init__(self, table, V: int, n_states: int, row_start):
        self.table, self.V, self.n_states, self.row_start = table, int(V), int(n_states), row_start

    @property
    def rows(self) -> int:
        return int(self.row_start.numel())


class ConstraintPool:
    """The constraints of one `generate_many` call as ONE device table: the `with_eos(eos_ids)` tables of the distinct constraints (distinct
    by identity: the same object is stored once) one behind the other, NOT renumbered - a state keeps the number it has in its own
    constraint, and a row is told where its table begins (`base`) and how many states it has (ops.SlotConstraints, the per-row pick).
    MAX_STATES therefore bounds each constraint, not the pool.  Pure host code apart from `bind`'s one upload.

    constraints: one entry per request, a TokenConstraint or None (an unconstrained request).  For request i:
      base[i], n_states[i], start[i]   the pool row of its state 0, its number of states, its start state; (0, 0, -1) without a constraint
    total_states: the pool's rows; nbytes: what `bind` uploads, total_states * ld * 2 with ld = V rounded up to a multiple of 8.
    V: the logits' width, which every constraint has to be built for.  Every failed check is a ValueError that names the first request
    using the constraint; so is nbytes > max_table_bytes, with the byte count."""

    def __init__(self, eos_ids, constraints: Sequence[Optional[TokenConstraint]], V: int, max_table_bytes: int = DEFAULT_MAX_TABLE_BYTES):
        self.V, self.ld = int(V), (int(V) + 7) // 8 * 8
        self.eos = sorted({int(e) for e in (eos_ids or [])})
        self.members: List[TokenConstraint] = []
        self._tables: List[np.ndarray] = []
        self.base, self.n_states, self.start = [], [], []
        at, off = {}, 0                 # id(constraint) -> (base, n_states, start)
        for i, c in enumerate(constraints):
            if c is None:
                self.base.append(0), self.n_states.append(0), self.start.append(-1)
                continue
            if id(c) not in at:
                who = f"request {i}"
                if not isinstance(c, TokenConstraint):
                    raise ValueError(f"{who}: constraint is an aki_amd.TokenConstraint, got {type(c).__name__}")
                if len(c.starts) != 1:
                    raise ValueError(f"{who}: a constraint with {len(c.starts)} start states; a request has one row, so exactly one is expected")
                if c.V != self.V:
                    raise ValueError(f"{who}: the constraint was built for V = {c.V}, the logits have {self.V} columns")
                if c.n_states > MAX_STATES:
                    raise ValueError(f"{who}: a token constraint holds at most {MAX_STATES} states, got {c.n_states}")
                try:
                    table = c.with_eos(self.eos)
                except ValueError as e:
                    raise ValueError(f"{who}: {e}") from None
                at[id(c)] = (off, c.n_states, c.starts[0])
                self.members.append(c)
                self._tables.append(table)
                off += c.n_states
            b, n, s = at[id(c)]
            self.base.append(b), self.n_states.append(n), self.start.append(s)
        self.total_states = off
        self.nbytes = self.total_states * self.ld * 2
        if self.nbytes > int(max_table_bytes):
            raise ValueError(f"the constraints' device table needs {self.total_states} * {self.ld} * 2 = {self.nbytes} bytes, above "
                             f"max_table_bytes = {int(max_table_bytes)}")

    @property
    def constrained(self) -> bool:
        return self.total_states > 0

    def table(self) -> np.ndarray:
        """The pool on the host, int32 [total_states, V]: the members' with_eos tables concatenated as they are."""
        return np.concatenate(self._tables, axis=0) if self._tables else np.zeros((0, self.V), dtype=np.int32)

    def bind(self, device):
        """The pool on `device`, uploaded once: int16 [total_states, ld], the columns behind V filled with -1."""
        if not self.constrained:
            raise ValueError("ConstraintPool.bind: no request of the call is constrained")
        import torch
        host = np.empty((self.total_states, self.ld), dtype=np.int16)
        host[:, self.V:] = -1
        off = 0
        for t in self._tables:                      # straight into the int16 rows: no int32 copy of the whole pool on the way
            host[off:off + t.shape[0], :self.V] = t
            off += t.shape[0]
        return torch.from_numpy(host).to(device)


def constraint_for_rows(constraint, B: int, n_ret: int = 1):
    """generate's `constraint` keyword - one TokenConstraint for every sample, or a list of B of them - as (one TokenConstraint, the start
    state of each of the B * n_ret rows): row b * n_ret + j continues sample b."""
    if isinstance(constraint, TokenConstraint):
        if len(constraint.starts) != 1:
            raise ValueError(f"a constraint with {len(constraint.starts)} start states: pass a list with one constraint per sample instead")
        return constraint, [constraint.starts[0]] * (B * n_ret)
    members: List[TokenConstraint] = list(constraint)
    if len(members) != B or any(not isinstance(m, TokenConstraint) or len(m.starts) != 1 for m in members):
        raise ValueError(f"constraint is a TokenConstraint or a list of one per sample (B = {B}), each with one start state; got {len(members)}")
    u = TokenConstraint.union(members)
    return u, [u.starts[b] for b in range(B) for _ in range(n_ret)]
