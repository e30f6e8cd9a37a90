"""Stand-in for verifiable_mpc/ac20/nullity.py: same names and call signatures (nullity.py:21-40), own code, over this
package's stand-in pivots.  The amortised form is built by Horner's rule over the caller's own form objects with the
challenge as a Python int - the same integer coefficients as the reference's sum of forms times powers - and the hash
is taken through the `pivot` MODULE OBJECT, which is where install() puts this package's function."""
from . import compressed_pivot, pivot


def _amortised(lin_forms, rho):
    forms = list(lin_forms)
    acc = forms[-1] * 1
    for form in reversed(forms[:-1]):
        acc = form + acc * rho
    return acc


def prove_nullity_compressed(generators, P, lin_forms, x, gamma, gf):
    rho = pivot.fiat_shamir_hash([P, lin_forms], gf.order)
    L = _amortised(lin_forms, rho)
    y = L(x)
    return compressed_pivot.protocol_5_prover(generators, P, L, y, x, gamma, gf), L, y, rho


def verify_nullity_compressed(generators, P, L, lin_forms, rho, y, proof, gf):
    if not _amortised(lin_forms, rho) == L:
        print("Linear form L does not correspond to reconstructed linear form with rho.")
        return False
    return compressed_pivot.protocol_5_verifier(generators, P, L, y, proof, gf)
