"""Case tables and the numpy reference of the per-request logits processors of generate_many (aki_amd/slots.py: RequestParams' processor
fields, resolve_processors, processor_set_key; ops.ProcessorSets; the per-row entry points aki_logits_process_rows / aki_greedy_pick_rows /
aki_sample_pick_rows_processed in aki_amd/csrc/decode.hip).

numpy only.  tests/test_many_processors_cpu.py checks the reference against the installed transformers' processors and the host half;
tests/test_many_processors_gpu.py runs the tables on the device.

A SET is slots.processor_set_key's value: (penalty, ngram, min_len, suppress ids, begin-suppress ids, bad words)."""
import numpy as np

EOS = (2, 31)                       # inside every width of the tables, and inside the histories' alphabet
PAD = 3
HISTORY = 40                        # columns of the token history; the pick writes column n <= 39
ALPHABET = 24                       # the histories draw from [0, 24): repeats, matching n-grams and bad-word prefixes are common
WIDTHS = (1000, 32064, 32066)       # a small row; the vector path; an odd width (stored with a padded row stride)

NEUTRAL = (1.0, 0, 0, (), (), ())
SETS = {
    "neutral": NEUTRAL,
    "penalty": (1.3, 0, 0, (), (), ()),
    "bigram_words": (0.7, 2, 0, (), (), ((5,), (9, 11), (4, 4, 6))),
    "all": (1.2, 3, 6, (13, 17), (19, 20), ((7, 3),)),
    "unigram": (1.0, 1, 0, (), (), ()),
}
# the two orders the pool is built in: where a set lies must not matter (the neutral set is always first)
ORDERS = (("penalty", "bigram_words", "all", "unigram"), ("unigram", "all", "bigram_words", "penalty"))

OUT_OF_RANGE = "out of range"       # a row whose set index lies outside the pool: processed with the neutral set
# (set, generated-token index n, finished): B = 6 rows, every n of {0, 1, 7, 23, 39} on a processed row in one table or the other
TABLES = {
    "a": (("neutral", 23, False), ("all", 1, True), (OUT_OF_RANGE, 39, False), ("all", 0, False), ("bigram_words", 39, False),
          ("penalty", 7, False)),
    "b": (("bigram_words", 7, False), ("unigram", 1, False), ("all", 23, False), ("neutral", 0, False), ("penalty", 39, True),
          (OUT_OF_RANGE, 7, False)),
}
START = 100                         # start_len of every row: the prompt's rows in the cache


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32)


def histories(B, seed):
    """int64 [B, HISTORY]: the recipe of tests/test_logits_processors_gpu.py - a small alphabet, a planted bad word (4, 4, 6) and, in row
    1, a planted repeated bigram."""
    g = np.random.default_rng(seed)
    h = g.integers(0, ALPHABET, (B, HISTORY)).astype(np.int64)
    h[:, 5:8] = (4, 4, 6)
    if B > 1:
        h[1, 10:12] = h[1, 20:22]
    return h


def logits(table, V, seed):
    """bf16-exact f32 [B, V].  Two rows are steered: the first unfinished "penalty" row gets a dominant EOS[0] column (its pick ends the
    row), the first unfinished "all" row with n < its minimum length a dominant EOS[1] column (which the minimum length must ban)."""
    g = np.random.default_rng([seed, V])
    x = (g.standard_normal((len(table), V)) * 4).astype(np.float32)
    for want, col in (("penalty", EOS[0]), ("all", EOS[1])):
        for b, (name, n, fin) in enumerate(table):
            if name == want and not fin and (want == "penalty" or n < SETS["all"][2]):
                x[b, col] = 60.0
                break
    return bf16_round(x)


def reference_row(x, h, key, eos=EOS):
    """The six stages for one row: f32 scores x [V], the row's generated tokens h [n], its set -> the processed f32 scores, in the
    kernel's f32 arithmetic (one multiplication or division per distinct history token, then bans to -inf)."""
    pen, ngram, min_len, sup, bsup, words = key
    x = np.array(x, np.float32, copy=True)
    V, h = x.shape[0], np.asarray(h, np.int64)
    n = len(h)
    inside = lambda i: 0 <= int(i) < V
    if pen != 1.0 and n:
        u = np.unique(h[(h >= 0) & (h < V)])
        p = np.float32(pen)
        x[u] = np.where(x[u] < 0, x[u] * p, x[u] / p).astype(np.float32)
    banned = []
    if ngram > 0 and n + 1 >= ngram:
        tail = tuple(h[n - ngram + 1:])
        banned += [h[i + ngram - 1] for i in range(n - ngram + 1) if tuple(h[i:i + ngram - 1]) == tail]
    for w in words:
        L = len(w)
        if L == 1 or (L <= n and tuple(h[n - (L - 1):]) == tuple(w[:-1])):
            banned.append(w[-1])
    if n < min_len:
        banned += list(eos)
    banned += list(sup)
    if n == 0:
        banned += list(bsup)
    for i in banned:
        if inside(i):
            x[int(i)] = -np.inf
    return x


def pool_keys(order):
    return [SETS[name] for name in order]


def row_keys(table):
    """The set each row is PROCESSED with (the neutral set for the out-of-range row)."""
    return [NEUTRAL if name == OUT_OF_RANGE else SETS[name] for name, _, _ in table]


def reference(table, x, h):
    """[B, V] processed scores of the table's rows; a finished row is the plain copy."""
    return np.stack([x[b] if fin else reference_row(x[b], h[b, :n], key) for b, ((_, n, fin), key) in enumerate(zip(table, row_keys(table)))])


def hf_kwargs(key, eos=EOS):
    """The keywords tests/test_logits_processors_gpu.py's hf_processors takes for a set."""
    pen, ngram, min_len, sup, bsup, words = key
    return dict(penalty=pen, ngram=ngram, bad=[list(w) for w in words] or None, min_new=min_len, eos=tuple(eos), suppress=list(sup) or None,
                begin_suppress=list(bsup) or None)


# ---- the end-to-end queue on the tiny model: RequestParams keywords per request (None: nothing of its own) --------------------------------
BUDGETS = [12, 1, 5, 12, 3, 9, 12]  # tests/test_slots_gpu.py's, restated: this file imports no torch
NGRAM2, NOTHING, SUPPRESS, BEGIN, EXPLICIT_NEUTRAL, WORDS, HEAVY = range(7)


def request_settings(plain):
    """Seven requests' own processor keywords (None: a request that sets nothing), the long budgets on the requests whose settings need
    room.  plain[r]: the plain run's tokens of request r (a list) - the suppressions aim at what the plain run really emits."""
    return [dict(repetition_penalty=1.3, no_repeat_ngram_size=2),
            None,
            dict(suppress_tokens=sorted(set(plain[2][:3]))),
            dict(begin_suppress_tokens=[plain[3][0]]),
            dict(repetition_penalty=1.0),
            dict(no_repeat_ngram_size=2, bad_words_ids=[[plain[5][0]], list(plain[5][1:3])]),
            dict(repetition_penalty=1.5, no_repeat_ngram_size=3, suppress_tokens=[plain[6][1]])]


def repeated_ngrams(row, n):
    grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
    return len(grams) - len(set(grams))
