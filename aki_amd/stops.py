"""Stop sequences for generate and generate_many: the host side (ops.stop_check / ops.slot_tick(stops=...) are the device side).

A *stop set* is an ordered list of at most STOP_MAX_SEQS token-id sequences, each of 1 to STOP_MAX_LEN ids in [0, V).  A live row finishes at
the first generated-token index t at which some sequence s of its set matches: with n = len(s), n <= t + 1 and tokens[t - n + 1 .. t] == s.
Only generated tokens count - never the prompt, never what an earlier request left in a refilled slot.  The matched sequence stays in the
returned tokens, as an EOS does.  stop_hit is the index within the set of the LOWEST-numbered sequence that matched at that t, -1 for a row
that ended otherwise; a row the pick's EOS check ended at the same t keeps -1 (EOS wins a tie); a stop and the budget at the same t is a
stop.  Stops change when a row ends, never what it picks: they apply behind the pick and ignore min_length / min_new_tokens.

Nothing in this module touches a device unless it is handed device tensors."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

STOP_MAX_SEQS = 64                  # AKI_STOP_MAX_SEQS: sequences of one set, one lane of a wave each
STOP_MAX_LEN = 32                   # AKI_STOP_MAX_LEN: ids of one sequence


def _is_int(x) -> bool:
    if isinstance(x, bool):
        return False
    if isinstance(x, int):
        return True
    try:
        return float(x) == int(x)
    except (TypeError, ValueError, OverflowError):
        return False


def check_stop_sequences(who: str, value, V: Optional[int] = None) -> Tuple[Tuple[int, ...], ...]:
    """A stop set, checked -> its normal form, a tuple of tuples of ints (order kept: it defines stop_hit).  ValueError beginning with
    `who` for a value that is not a list of non-empty lists of integer ids, an id outside [0, V) (V, the logits' width, bounds the ids when
    it is known), more than STOP_MAX_SEQS sequences, or a sequence longer than STOP_MAX_LEN ids.  [] and () are the empty set."""
    shape = f"{who}: stop_sequences has to be a list of non-empty lists of token ids, got {value!r}"
    if value is None or isinstance(value, (str, bytes)) or not hasattr(value, "__iter__"):
        raise ValueError(shape)
    out = []
    for s in value:
        if isinstance(s, (str, bytes)) or not hasattr(s, "__iter__") or not hasattr(s, "__len__") or len(s) == 0:
            raise ValueError(shape)
        seq = []
        for i in s:
            if not _is_int(i):
                raise ValueError(f"{who}: stop_sequences: a token id is an integer, got {i!r}")
            i = int(i)
            if i < 0 or (V is not None and i >= int(V)):
                raise ValueError(f"{who}: stop_sequences: every id has to be in [0, {'V' if V is None else int(V)}), got {i}")
            seq.append(i)
        if len(seq) > STOP_MAX_LEN:
            raise ValueError(f"{who}: stop_sequences: a sequence of {len(seq)} ids; at most {STOP_MAX_LEN} are served")
        out.append(tuple(seq))
    if len(out) > STOP_MAX_SEQS:
        raise ValueError(f"{who}: stop_sequences: {len(out)} sequences; at most {STOP_MAX_SEQS} are served")
    return tuple(out)


def resolve_stop_sequences(own, default, call):
    """One request's stop set: its own RequestParams.stop_sequences, else that of `default` (generate_many's params=), else the call-wide
    keyword's value `call`.  Only None passes a level on: () means the request has none.  The value is returned as it stands (not yet
    checked); None when no level sets one."""
    for v in (own, default, call):
        if v is not None:
            return v
    return None


class StopPool:
    """The distinct stop sets of a call, deduplicated by value (order inside a set is significant), as the arrays the kernels read:
      keys       the sets in their normal form; keys[0] is always the empty set
      index      {key: its place in the pool}
      ids        every sequence one behind the other
      seq_off    [n_seqs + 1]: sequence s is ids[seq_off[s] : seq_off[s + 1]]
      set_first  [n_sets + 1]: the sequences of set k are set_first[k] .. set_first[k + 1]
    All Python lists: the layout is checked without a device."""

    def __init__(self, sets: Sequence):
        self.keys = [()]
        for k in sets:
            k = check_stop_sequences("stop pool", k)
            if k not in self.keys:
                self.keys.append(k)
        self.index = {k: i for i, k in enumerate(self.keys)}
        self.ids, self.seq_off, self.set_first = [], [0], [0]
        for k in self.keys:
            for s in k:
                self.ids += list(s)
                self.seq_off.append(len(self.ids))
            self.set_first.append(len(self.seq_off) - 1)

    @property
    def n_sets(self) -> int:
        return len(self.keys)

    @property
    def n_seqs(self) -> int:
        return len(self.seq_off) - 1


def first_finish(tokens, eos_t, sets: Sequence, row_set: Sequence[int]):
    """The rule above for whole rows, in torch on the tokens' device, without a synchronisation.  tokens int64 [B, n]: each row's generated
    tokens from index 0; eos_t: the eos ids as an int64 tensor [E] or None; sets: stop sets in their normal form; row_set: for each row
    the place of its set in `sets` (a place outside it: no stops).  Returns (finished [B] bool: an EOS or a stop sequence ends the row inside
    these n tokens; index [B] int64 of the token that ends it, 0 where nothing does; hit [B] int32: the lowest-numbered sequence that
    matched at that index, -1 where the row is not finished or its EOS ended it - EOS wins a tie)."""
    import torch
    B, n = tokens.shape
    dev = tokens.device
    never = torch.full((B,), n, dtype=torch.long, device=dev)
    col = torch.arange(n, device=dev)
    eos_pos = never
    if eos_t is not None and n > 0:
        is_eos = (tokens[:, :, None] == eos_t[None, None, :]).any(-1)
        eos_pos = torch.where(is_eos, col[None, :], never[:, None]).min(1).values
    stop_pos, hit = never, torch.full((B,), -1, dtype=torch.int32, device=dev)
    row_set = [int(k) for k in row_set]
    if len(row_set) != B:
        raise ValueError(f"first_finish: {len(row_set)} set indices for {B} rows")
    for k in sorted(set(row_set)):
        if not 0 <= k < len(sets) or not sets[k]:
            continue
        rows = None if all(r == k for r in row_set) else torch.tensor([r == k for r in row_set], dtype=torch.bool, device=dev)
        for j, s in enumerate(sets[k]):
            m = len(s)
            if m > n:
                continue
            w = n - m + 1                               # the windows tokens[:, a : a + m], a < w; a match ends at a + m - 1 >= m - 1
            match = tokens[:, 0:w] == int(s[0])
            for i in range(1, m):
                match = match & (tokens[:, i:i + w] == int(s[i]))
            if rows is not None:
                match = match & rows[:, None]
            pos = torch.where(match, col[None, :w] + (m - 1), never[:, None]).min(1).values
            better = pos < stop_pos                     # strictly: among the sequences that match at one index the lowest number stays
            hit = torch.where(better, torch.full_like(hit, j), hit)
            stop_pos = torch.where(better, pos, stop_pos)
    index = torch.minimum(eos_pos, stop_pos)
    finished = index < n
    by_stop = finished & (stop_pos < eos_pos)
    return finished, torch.where(finished, index, torch.zeros_like(index)), torch.where(by_stop, hit, torch.full_like(hit, -1))
