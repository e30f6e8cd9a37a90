"""A big-int restatement of the R1CS solve on Shamir shares (verifiable_mpc_amd/pynocchio.py ShareSolvePlan,
csrc/r1cs_share.h, trinocchio.calculate_witness_shares), written from the definitions: which row
defines which wire comes from tests/witness_ref.plan, the classification, the depth mu (a fixpoint over ALL rows, no
order assumed), the phases and the M-party solve are stated here on Python ints; and a generator of circuits with
prescribed product-round widths and linear sub-level depths.  The independent side of
tests/test_witness_share_plan_host.py and tests/test_gpu_witness_shares.py.

An R1CS is tests/witness_ref's (V, W, Y, m)."""
import random

from tests import witness_ref as WR

N = WR.N
CHECK, KY, KA, KB = WR.CHECK, WR.KY, WR.KA, WR.KB


class SharedDivisor(ValueError):
    pass


class ZeroDivisor(ValueError):
    pass


def _shared(mat):
    return any(w != 0 for w in mat)


def classify(r1cs, n_in):
    """-> (defining rows, n_checks); a defining row is a dict: row (0-based), kind, wire, inv, mats [a, b, y] as
    {wire: coefficient} without the new wire, product (bool).  Raises SharedDivisor / ZeroDivisor with .args[1] the
    1-based constraint."""
    out, checks = [], 0
    for level in WR.plan(r1cs, n_in):
        for j, kind, s, inv, mats in level:
            if kind == CHECK:
                checks += 1
                continue
            product = False
            if kind == KY:
                product = _shared(mats[0]) and _shared(mats[1])
            else:
                div = mats[1] if kind == KA else mats[0]
                if _shared(div):
                    raise SharedDivisor("division by a shared value", j + 1)
                if div.get(0, 0) % N == 0:
                    raise ZeroDivisor("division by the constant 0", j + 1)
            out.append(dict(row=j, kind=kind, wire=s, inv=inv, mats=mats, product=product))
    return out, checks


def depths(rows, n_in):
    """mu per wire by fixpoint: every pass looks at every row that has no depth yet"""
    mu = {w: 0 for w in range(n_in + 1)}
    todo = list(rows)
    while todo:
        rest = []
        for x in todo:
            read = [w for mat in x["mats"] for w in mat]
            if all(w in mu for w in read):
                mu[x["wire"]] = max([mu[w] for w in read], default=0) + (1 if x["product"] else 0)
            else:
                rest.append(x)
        assert len(rest) < len(todo), "a row reads a wire that nothing defines"
        todo = rest
    return mu


def phases(r1cs, n_in):
    """-> (list of phases in solve order, n_checks): ("L", r, [sub-levels, each a list of defining rows]) and
    ("P", r, [defining rows]), L_0, P_1, L_1, .., P_D, L_D, rows in ascending row index"""
    rows, checks = classify(r1cs, n_in)
    mu = depths(rows, n_in)
    D = max(mu.values())
    linear_wires = {x["wire"] for x in rows if not x["product"]}
    sub = {}
    todo = [x for x in rows if not x["product"]]
    while todo:                                          # sub-levels by fixpoint as well
        rest = []
        for x in todo:
            r = mu[x["wire"]]
            same = [w for mat in x["mats"] for w in mat if w in linear_wires and mu[w] == r]
            if all(w in sub for w in same):
                sub[x["wire"]] = max([sub[w] + 1 for w in same], default=0)
            else:
                rest.append(x)
        assert len(rest) < len(todo)
        todo = rest
    out = []
    for r in range(D + 1):
        if r:
            out.append(("P", r, sorted((x for x in rows if x["product"] and mu[x["wire"]] == r), key=lambda x: x["row"])))
        mine = [x for x in rows if not x["product"] and mu[x["wire"]] == r]
        levels = []
        for k in range(max([sub[x["wire"]] for x in mine], default=-1) + 1):
            levels.append(sorted((x for x in mine if sub[x["wire"]] == k), key=lambda x: x["row"]))
        out.append(("L", r, levels))
    return out, checks


def round_widths(ph):
    return [len(p[2]) for p in ph if p[0] == "P"]


def local_depths(ph):
    return [len(p[2]) for p in ph if p[0] == "L"]


# ---- the arithmetic of one element ------------------------------------------------------------------------------------

def dot(mat, c):
    return sum(x * c[w] for w, x in mat.items()) % N


def linear_value(x, c):
    """the row's own formula on a (share) vector c"""
    a, b, y = (dot(mat, c) for mat in x["mats"])
    if x["kind"] == KY:
        return (a * b - y) * x["inv"] % N
    div, rest = (b, a) if x["kind"] == KA else (a, b)
    return (y * pow(div, -1, N) - rest) * x["inv"] % N


def deal_element(x, c, coeffs, parties):
    """what a party with the share vector c deals for the product row x: [d + sum_k coeffs[k-1] (q+1)^k for q]"""
    d = dot(x["mats"][0], c) * dot(x["mats"][1], c) % N
    return [(d + sum(ck * pow(q + 1, k + 1, N) for k, ck in enumerate(coeffs))) % N for q in range(parties)]


def finish_element(x, c, parts, weights):
    """the new wire from the M values that arrived"""
    s = sum(wt * v for wt, v in zip(weights, parts)) % N
    return (s - dot(x["mats"][2], c)) * x["inv"] % N


def lagrange_at_zero(xs):
    out = []
    for i, xi in enumerate(xs):
        num = den = 1
        for j, xj in enumerate(xs):
            if i != j:
                num = num * (-xj) % N
                den = den * (xi - xj) % N
        out.append(num * pow(den, -1, N) % N)
    return out


def share(values, t, parties, rng):
    """degree-t Shamir shares of each value: shares[p][i], party p at node p + 1"""
    polys = [[v % N] + [rng.randrange(N) for _ in range(t)] for v in values]
    return [[sum(ck * pow(p + 1, k, N) for k, ck in enumerate(poly)) % N for poly in polys] for p in range(parties)]


def recombine(shares, nodes):
    """the value at 0 of the polynomial through (nodes[i], shares[i])"""
    return sum(l * s for l, s in zip(lagrange_at_zero(nodes), shares)) % N


def solve_shares(r1cs, x_shares, t, coeff):
    """all M parties at once: x_shares[p] = party p's shares of the inputs; coeff(p, r, k, i) = the coefficient of
    x^k (k = 1 .. t) that party p deals for the i-th product row of round r.  -> c[p] = party p's shares of every wire
    (c[p][0] = 1), and the number of rounds"""
    M, n_in = len(x_shares), len(x_shares[0])
    ph, _ = phases(r1cs, n_in)
    weights = lagrange_at_zero(list(range(1, M + 1)))
    c = [{0: 1, **{1 + i: v % N for i, v in enumerate(xs)}} for xs in x_shares]
    for what, r, body in ph:
        if what == "L":
            for level in body:
                new = [[(x["wire"], linear_value(x, c[p])) for x in level] for p in range(M)]
                for p in range(M):
                    c[p].update(new[p])
            continue
        dealt = [[deal_element(x, c[p], [coeff(p, r, k, i) for k in range(1, t + 1)], M) for i, x in enumerate(body)]
                 for p in range(M)]
        for q in range(M):
            c[q].update({x["wire"]: finish_element(x, c[q], [dealt[p][i][q] for p in range(M)], weights)
                         for i, x in enumerate(body)})
    m = r1cs[3]
    return [[cp[w] for w in range(m + 1)] for cp in c], len(round_widths(ph))


# ---- circuits with prescribed rounds --------------------------------------------------------------------------------

def share_layered_r1cs(widths, local, seed, n_in=2, local_width=3):
    """A solvable R1CS whose share plan has exactly the product-round widths `widths` (round r = 1 .. D has widths[r-1]
    product rows) and local[r] linear sub-levels in L_r (len(local) == len(widths) + 1; 0: an empty phase), each of 1 ..
    local_width rows.  Every product row reads a wire of depth r - 1 in V and a shared wire in W; sub-level 0 of L_r
    reads a product wire of round r (an input for r = 0), sub-level k a linear wire of sub-level k - 1.  Linear rows
    take the shapes constant * form = form + wire (either side the constant), the flattener's `set` row and a division
    by a constant (KIND_A and KIND_B).  Coefficients are small, negative, full size or >= N; a form never names a wire
    twice.  Rows shuffled.  -> (V, W, Y, m)"""
    assert len(local) == len(widths) + 1
    rng = random.Random(seed)
    coef = lambda: rng.choice([rng.randint(1, 3), -rng.randint(1, 3), rng.randrange(1, N), N + rng.randint(1, 5)])
    info = {i: (0, None) for i in range(1, n_in + 1)}        # wire -> (mu, linear sub-level or None)
    rows, nxt = [], n_in + 1

    def form(allowed, must=None, extra=2):
        wires = rng.sample(allowed, min(len(allowed), rng.randint(0, extra)))
        if must is not None and must not in wires:
            wires.append(must)
        f = [(w, coef()) for w in wires]
        rng.shuffle(f)
        return f

    def linear_phase(r, n_sub):
        nonlocal nxt
        for k in range(n_sub):
            if k == 0:
                musts = [w for w, (mu, sub) in info.items() if mu == r and sub is None]
            else:
                musts = [w for w, (mu, sub) in info.items() if mu == r and sub == k - 1]
            allowed = [0] + [w for w, (mu, sub) in info.items() if mu < r or (mu == r and (sub is None or sub < k))]
            new = []
            for _ in range(rng.randint(1, local_width)):
                s, nxt = nxt, nxt + 1
                lin, const = form(allowed, rng.choice(musts)), [(0, coef())]
                shape = rng.randrange(5)
                if shape == 0:
                    row = (const, lin, form(allowed) + [(s, coef())])
                elif shape == 1:
                    row = (lin, const, form(allowed) + [(s, coef())])
                elif shape == 2:                             # set: (s - form) * 1 = nothing
                    row = (lin + [(s, 1)], [(0, 1)], [])
                elif shape == 3:                             # (k s + form) * const = form: a division by a constant
                    row = (form(allowed) + [(s, coef())], const, lin)
                else:
                    row = (const, form(allowed) + [(s, coef())], lin)
                rows.append(row)
                new.append(s)
            for s in new:
                info[s] = (r, k)

    linear_phase(0, local[0])
    for r, width in enumerate(widths, start=1):
        musts = [w for w, (mu, _) in info.items() if mu == r - 1]
        allowed = [0] + list(info)                           # everything so far has depth < r
        shared = list(info)
        new = []
        for _ in range(width):
            s, nxt = nxt, nxt + 1
            rows.append((form(allowed, rng.choice(musts)), form(allowed, rng.choice(shared)),
                         form(allowed, extra=1) + [(s, coef())]))
            new.append(s)
        for s in new:
            info[s] = (r, None)
        linear_phase(r, local[r])
    rng.shuffle(rows)
    V, W, Y = ([row[k] for row in rows] for k in range(3))
    return V, W, Y, nxt - 1
