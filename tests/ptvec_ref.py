"""The element-wise Ed25519 point-vector operations of csrc/exact.hip and csrc/msm.hip on Python ints: what
tests/test_gpu_point_vectors.py holds the kernels against where oracle/ed25519_ref.py has no function of its own.
Written from include/vmpc.h and the kernels' stated contracts; nothing of the package under test is imported.

    normalize           (X : Y : Z) -> (X / Z, Y / Z), and (0, 0) for Z = 0: such a triple is no point, and (0, 0) is
                        what no validation accepts
    rescale             (lam X : lam Y : lam Z), another representative of the same group element
    is_valid_affine     what vmpc_points_validate_dev lets pass: both raw 256-bit values below p, and on the curve
                        (the subgroup is not looked at)
    sign_magnitude      the 32-byte exponent of vmpc_repeat_dev's mode 2: |n| < 2^255 in bits 0..254, bit 255 set for
                        n < 0; "-0" (the sign bit over a zero magnitude) is an encoding of 0
    LOW_ORDER           the points of order 1, 2 and 4: canonical and on the curve, so validation passes them
    affine_with_x / _y  the curve points with a given coordinate, for encodings like x + p that need a small one

repeat, fold and tree_reduce are ed.pt_repeat, ac20_ref.fold_generators and ed.tree_reduce.
"""
from oracle import ed25519_ref as ed

P, ELL, D = ed.P, ed.ELL, ed.D

LOW_ORDER = [(0, 1), (0, P - 1), (ed.SQRT_M1, 0), (P - ed.SQRT_M1, 0)]


def normalize(points):
    out = []
    for x, y, z in points:
        zi = pow(z % P, P - 2, P)           # 0 for Z = 0
        out.append((x * zi % P, y * zi % P) if z % P else (0, 0))
    return out


def rescale(point, lam):
    assert lam % P
    return tuple(c * lam % P for c in point)


def is_valid_affine(x_raw, y_raw):
    if not (0 <= x_raw < P and 0 <= y_raw < P):
        return False
    x2, y2 = x_raw * x_raw % P, y_raw * y_raw % P
    return (y2 - x2 - 1 - D * x2 % P * y2) % P == 0


def sign_magnitude(n, negative_zero=False):
    assert abs(n) < 1 << 255 and not (negative_zero and n)
    return (abs(n) | ((n < 0 or negative_zero) << 255)).to_bytes(32, "little")


def from_sign_magnitude(b):
    v = int.from_bytes(b, "little")
    mag = v & ((1 << 255) - 1)
    return -mag if v >> 255 else mag


def _sqrt(a):
    """a square root of a mod p (p = 5 mod 8), or None"""
    a %= P
    r = pow(a, (P + 3) // 8, P)
    if (r * r - a) % P:
        r = r * ed.SQRT_M1 % P
    return r if (r * r - a) % P == 0 else None


def affine_with_x(x):
    """(x, y) on -x^2 + y^2 = 1 + d x^2 y^2, or None: y^2 = (1 + x^2) / (1 - d x^2)"""
    y = _sqrt((1 + x * x) * pow(1 - D * x * x, P - 2, P))
    return None if y is None else (x % P, y)


def affine_with_y(y):
    """x^2 = (y^2 - 1) / (d y^2 + 1)"""
    x = _sqrt((y * y - 1) * pow(D * y * y + 1, P - 2, P))
    return None if x is None else (x, y % P)
