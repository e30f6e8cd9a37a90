"""Inputs for the BN-256 MSM edge tests (tests/test_gpu_bn256_edges.py), checked on the CPU by
tests/test_bn256_msm_inputs.py.

Restates, in Python, what the planner and the recoding of csrc/msm_sort.hip decide for a BN-256 MSM
(256-bit scalars, modulus = the group order N):
    msm_pick_window / msm_make_plan   window width c and window count W
    msm_recode_term                   the signed digits, carry included
    msm_plan_geometry, bn_reduce_split  whether gk_reduce runs with one or two lanes per chunk
and builds the scalar vectors that drive the kernels into their extreme buckets and coincidences.
"""
import collections
import random

from oracle import bn256_ref as bn

N = bn.N
SCALAR_BITS = 256
MAX_C = 16                  # MSM_MAX_C
MSM_SEG = 64                # MSM_SEG: a segment holds MSM_SEG << seg_shift entries, seg_shift <= 4
MAX_SEG_LEN = MSM_SEG << 4
FINISH_SERIAL = 32          # MSM_FINISH_SERIAL: buckets split more ways go through gk_finish's workgroup tree
REDUCE_CHUNKS = 4096        # MSM_REDUCE_CHUNKS
REDUCE_MAX_CHUNKS = 32768   # vmpc_ctx::reduce_max_chunks default
TABLE_C, TABLE_W = 16, 17   # BN_TABLE_C, BN_TABLE_W


def pick_window(n):
    """msm_pick_window for 256-bit scalars: the cost model W * (n + 2.5 * 2^(c-1))"""
    best, best_c = None, 4
    for c in range(4, MAX_C + 1):
        W = (SCALAR_BITS + 2 + c - 1) // c
        cost = W * (n + 2.5 * (1 << (c - 1)))
        if best is None or cost < best:
            best, best_c = cost, c
    return best_c


def make_plan(n, window=0):
    """(c, W) of msm_make_plan; `window` is vmpc_ctx_set_window's override (0: the planner picks)"""
    c = window if window else pick_window(n)
    c = min(max(c, 4), MAX_C)
    W = (SCALAR_BITS + 2 + c - 1) // c
    while W > 64:           # one lane per window in the recombination
        c += 1
        W = (SCALAR_BITS + 2 + c - 1) // c
    return c, W


def reduce_chunks(c, W):
    """msm_plan_geometry's chunk-lanes per window (default context, not a wide plan)"""
    nb = 1 << (c - 1)
    chunks = REDUCE_CHUNKS
    while chunks * 2 * W <= REDUCE_CHUNKS * 16 and chunks * 2 <= REDUCE_MAX_CHUNKS:
        chunks *= 2
    while chunks * W > REDUCE_CHUNKS * 16 and chunks > 256:
        chunks //= 2
    return min(chunks, nb)


def reduce_split(c, W, K=None):
    """1 or 2: gk_reduce<SPLIT> as bn_reduce_split picks it.  W windows of a variable-base plan; K (not None) is a
    multi-key pass over K tables (c = 16, one window each, chunk-lanes cut down for K windows as in bn256.hip)."""
    chunks = reduce_chunks(c, W)
    if K is not None:
        while chunks * K > REDUCE_CHUNKS * 16 and chunks > 256:
            chunks //= 2
        W = K
    ok = chunks * W <= 32768 and chunks >= 512 and chunks & (chunks - 1) == 0 and chunks % 128 == 0
    return 2 if ok else 1


def recode(s, c, W):
    """msm_recode_term: W signed digits in [-2^(c-1), 2^(c-1)); a non-canonical scalar (s >= N) counts as zero"""
    if s >= N:
        s = 0
    half, digits, carry = 1 << (c - 1), [], 0
    for _ in range(W):
        raw = (s & ((1 << c) - 1)) + carry
        if raw >= half:
            digits.append(raw - (1 << c))
            carry = 1
        else:
            digits.append(raw)
            carry = 0
        s >>= c
    return digits


def carry_into(s, c, k):
    """the carry the recoding brings into window k: a closed form, ((s mod 2^(ck)) + H_k) >> ck with
    H_k = sum_{j<k} 2^(c-1) 2^(cj) - monotone in the lower part s mod 2^(ck)"""
    H = sum((1 << (c - 1)) << (c * j) for j in range(k))
    return ((s & ((1 << (c * k)) - 1)) + H) >> (c * k)


def top_max_bucket(c, W):
    """msm_top_max_bucket: the planner's bound on the top window's bucket index, (N - 1) >> c(W - 1)"""
    return (N - 1) >> (c * (W - 1))


def extreme(c):
    """E_c = 2^(c-1) + sum_{w=1}^{W-2} (2^(c-1) - 1) 2^(cw): every digit below the top one is -2^(c-1) (the last
    bucket), the top digit 1"""
    _, W = make_plan(0, c)
    return (1 << (c - 1)) + sum(((1 << (c - 1)) - 1) << (c * w) for w in range(1, W - 1))


def bucket_counts(scalars, c, W, rows=1):
    """entries per bucket index |digit| of one bucket set: a plain MSM sorts each window into its own set (rows = 1:
    the largest count over the windows), a c = 16 table puts its `rows` rows into ONE set (rows = W = 17)"""
    per_window = [{} for _ in range(W)]
    for s, mult in collections.Counter(scalars).items():
        for w, d in enumerate(recode(s, c, W)):
            if d:
                per_window[w][abs(d)] = per_window[w].get(abs(d), 0) + mult
    out = {}
    for cnt in per_window:
        for d, v in cnt.items():
            out[d] = max(out.get(d, 0), v) if rows == 1 else out.get(d, 0) + v
    return out


# ---- scalar vectors --------------------------------------------------------------------------------------------

def wire_like(n, seed):
    """a witness as circuits make them: 54 % zeros, 9 % in {1, 2}, 5 % N - 1, 12 % small values below 2^16,
    5 % N - k for small k, the rest (15 %) uniform"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        u = rng.random()
        if u < 0.54:
            out.append(0)
        elif u < 0.63:
            out.append(rng.choice((1, 2)))
        elif u < 0.68:
            out.append(N - 1)
        elif u < 0.80:
            out.append(rng.randrange(1 << 16))
        elif u < 0.85:
            out.append(N - rng.randrange(2, 1000))
        else:
            out.append(rng.randrange(N))
    return out


def skewed_vectors(n, c, seed):
    """the skewed scalar vectors of an n-term MSM whose recoding uses width c: name -> list of n ints.
    'repeated' and 'extreme' are the heavy ones (one bucket takes every term of a window)."""
    rng = random.Random(seed)
    a, b = rng.randrange(1, N), rng.randrange(1, N)
    single = [0] * n
    single[rng.randrange(n)] = rng.randrange(1, N)
    return {
        "repeated": [rng.randrange(1, N)] * n,
        "extreme": [extreme(c)] * n,
        "wire": wire_like(n, seed + 1),
        "alternating": [a if i % 2 else b for i in range(n)],
        "single": single,
    }


HEAVY = ("repeated", "extreme")


def width_edge_scalars(c, rng, n):
    """~n scalars for a width-c run: E_c, N - 1, 2^(c-1) - 1, 2^(c-1), 2^(c-1) + 1, 0, then uniform"""
    head = [extreme(c), N - 1, (1 << (c - 1)) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, 0]
    return head + [rng.randrange(N) for _ in range(n - len(head))]
