"""Pi_Nullity (AC20 p. 17-18) on Python ints: the CPU restatement that tests/test_gpu_nullity.py holds
verifiable_mpc_amd.nullity and the kernels of csrc/nullity.hip against.  Forms are lists of coefficient lists.

    combine(forms, rho)         [sum_i rho^i forms[i][j] mod l]           (nullity.py:25)
    values(forms, x)            [sum_j forms[i][j] x[j] mod l]
    first_nonzero(forms, x)
    dense_digest / sparse_digest, compact_rho        the compact transcript
    reference_rho               int.from_bytes(SHA-256(str([P, lin_forms])), "little") mod l, the text restated
"""
import hashlib

ELL = 2**252 + 27742317777372353535851937790883648493
P25519 = 2**255 - 19
CHUNK = 4096


def combine(forms, rho, n=None):
    n = len(forms[0]) if forms else int(n or 0)
    out = [0] * n
    for i, form in enumerate(forms):
        w = pow(rho, i, ELL)
        for j, c in enumerate(form):
            out[j] = (out[j] + w * c) % ELL
    return out


def values(forms, x):
    return [sum(c * v for c, v in zip(form, x)) % ELL for form in forms]


def first_nonzero(forms, x):
    return next((i for i, v in enumerate(values(forms, x)) if v), None)


# ---- compact transcript -----------------------------------------------------------------------------------------------------
def dense_digest(forms, n=None):
    """SHA-256(b"vmpc-ac20/nullity/forms/v1" | b"D" | s u64 LE | n u64 LE | leaves): leaves = the SHA-256 of every
    4096-byte piece (the last may be short) of the s n canonical residues, 32 bytes little-endian each, row by row"""
    n = len(forms[0]) if forms else int(n or 0)
    data = b"".join((c % ELL).to_bytes(32, "little") for form in forms for c in form)
    leaves = b"".join(hashlib.sha256(data[o:o + CHUNK]).digest() for o in range(0, len(data), CHUNK))
    return hashlib.sha256(b"vmpc-ac20/nullity/forms/v1" + b"D" + len(forms).to_bytes(8, "little") +
                          n.to_bytes(8, "little") + leaves).digest()


def sparse_digest(rows, n):
    """rows: [{col: value}].  SHA-256(tag | b"S" | s u64 | n u64 | s u64 | nnz u64 | row_ptr (s + 1 u64) | cols (u64
    each) | values (32 B each) | s zero constants (32 B each)): entries sorted, zeros dropped (the canonical CSR bytes
    circuit_sat_gpu hashes for a circuit's matrices)"""
    canon = [sorted((c, v % ELL) for c, v in row.items() if v % ELL) for row in rows]
    ptr = [0]
    for e in canon:
        ptr.append(ptr[-1] + len(e))
    s = len(rows)
    h = hashlib.sha256(b"vmpc-ac20/nullity/forms/v1" + b"S" + s.to_bytes(8, "little") + n.to_bytes(8, "little"))
    h.update(s.to_bytes(8, "little") + ptr[-1].to_bytes(8, "little"))
    h.update(b"".join(p.to_bytes(8, "little") for p in ptr))
    h.update(b"".join(c.to_bytes(8, "little") for e in canon for c, _ in e))
    h.update(b"".join(v.to_bytes(32, "little") for e in canon for _, v in e))
    h.update(bytes(32 * s))
    return h.digest()


def compress(P_proj):
    """RFC 8032 encoding of the point (X : Y : Z)"""
    X, Y, Z = P_proj
    zi = pow(Z, P25519 - 2, P25519)
    x, y = X * zi % P25519, Y * zi % P25519
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def compact_rho(P_proj, forms_digest):
    return int.from_bytes(hashlib.sha256(b"vmpc-ac20/nullity/v1" + compress(P_proj) + forms_digest).digest(),
                          "little") % ELL


# ---- reference transcript -----------------------------------------------------------------------------------------------
def _signed(v, modulus):
    v %= modulus
    return v - modulus if v > modulus // 2 else v


def typed_text(t):
    """how a fixture's "i:<decimal>" (Python int) / "f:<hex>" (field element, printed signed) value prints"""
    return t[2:] if t[0] == "i" else str(_signed(int(t[2:], 16), ELL))


def reference_rho(P_proj, forms_typed):
    """the pre-image is str([P, lin_forms]): P as its three coordinates (residues mod 2^255 - 19 as they are), every
    form as "<coeffs>, 0" with field elements printed signed"""
    point = "[" + ", ".join(str(c % P25519) for c in P_proj) + "]"
    forms = ", ".join("[" + ", ".join(typed_text(t) for t in form) + "], 0" for form in forms_typed)
    text = "[" + point + ", [" + forms + "]]"
    return int.from_bytes(hashlib.sha256(text.encode("utf-8")).digest(), "little") % ELL


def typed_value(t):
    return int(t[2:]) if t[0] == "i" else int(t[2:], 16)
