"""Reference for vmpc_fr_batch_products_dev (csrc/batch_verify.hip) in Python ints, on tests.frvec_ref.challenge_products:

    u[j]    = sum_p w_p v_p[j]                           v_p = challenge_products(c_p, low_bits, z'_p)
    dots[p] = sum_{j < form_len} w_p v_p[j] forms[p][j]
"""
from tests import frvec_ref

ELL = frvec_ref.ELL


def batch_products(challenges, low_bits, zprimes, weights, forms, form_len):
    """challenges: K lists of R residues; zprimes: K lists of 2^low_bits; weights: K; forms: K lists of at least form_len
    residues (None where form_len == 0) -> (u, dots)"""
    K = len(challenges)
    assert K >= 1 and len(zprimes) == len(weights) == K
    n = 1 << (len(challenges[0]) + low_bits)
    assert 0 <= form_len <= n
    u, dots = [0] * n, []
    for p in range(K):
        v = frvec_ref.challenge_products(challenges[p], low_bits, zprimes[p])
        w = weights[p] % ELL
        u = [(a + w * b) % ELL for a, b in zip(u, v, strict=True)]
        dots.append(sum(w * v[j] * forms[p][j] for j in range(form_len)) % ELL)
    return u, dots
