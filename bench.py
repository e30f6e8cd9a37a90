#!/usr/bin/env python3
"""bench.py - Ed25519 MSM throughput (BASELINE.json metric) on N MI355X of one node.

One "step" = one Pedersen-commitment MSM (the hot loop of pivot.vector_commitment,
verifiable_mpc/ac20/pivot.py:143-144) over n = 2^20 terms PER GPU, inputs resident in HBM.
With --gpus N > 1 the N ranks hold the cyclic shards of one (N * 2^20)-term commitment: each
computes its partial point, one all-gather of the 128-byte extended points follows inside the
library (include/vmpc.h vmpc_comm_*: ncclAllGather on the MSM's own stream) and every rank adds
them in rank order ("weak" scaling).  The commitments of a launch are over DISTINCT
scalar vectors.  For N > 1 the result is checked across ranks (exponent identity), `"checked": true`.

Prints ONE JSON line (rank 0).  A plain run does only what the headline needs: it sets up, warms up,
times the K steps once, writes the last step's commitments if --dump-outputs DIR is given, and prints
the line.  Everything else is measured with --full: the median of --repeats (default 5) timed regions,
the result check, the other generator forms, `roofline` for the dominant kernel (k_msm_bucket, timed
with HIP events on the kernel's own stream, alone on the GPU after the timed region and inside it),
`cpu_baseline` (the C restatement of the REFERENCE algorithm - per-term double-and-add + product
tree - on one host core over a bounded sample), and at N = 1 the AC20 Protocol-5 prove time at
N = 2^20 in both transcript modes, other sizes and BN256 (extra keys, not the headline value); at
N > 1 the sharded prover's and config 4.  A run that makes no progress for --watchdog-s seconds
prints the line with an `error` entry and exits with status 3.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

# hardware queues for the HIP runtime (libvmpc_hip sets the same default when it is loaded - csrc/api.hip -; here too,
# because torch may initialise HIP first; with the default of 4 which streams run in order behind each other depends
# on how many were created before them)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
BYTES_PER_TERM = 96             # 32 B scalar + 64 B affine point


def rand_scalars(rng, n):
    """uniform in [0, 2^252) (< l), (n, 32) uint8 little-endian"""
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x0F
    return a


def pmc_traffic_calibrated(kernel):
    """HBM-side bytes per launch of `kernel` from the newest committed PMC summary (profiles/*_pmc_summary.json:
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes over this bench, scripts/profile_round.sh).  The
    FETCH_SIZE factor is the one measured IN THE SAME PASS on a gather of known size in this kernel's access
    pattern (vmpc_gather_probe_dev: one lane per random 128-byte line; scripts/traffic_calibration.py), not the
    guide's 2x for wide streaming reads.  The summary names the code revision it was taken on."""
    import glob
    out = {"bytes": None, "source": None, "detail": None}
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json")))
    if not files:
        return out
    try:
        with open(files[-1]) as f:
            d = json.load(f)
        k = d["kernels"].get(kernel)
        if not k:
            return out
        out["source"] = os.path.basename(files[-1])
        cal = d.get("calibrated", {}).get(kernel)
        if cal:
            out["bytes"] = cal["hbm_bytes_per_launch"]
            out["detail"] = {"FETCH_SIZE_KiB": k["FETCH_SIZE_KiB_avg"], "WRITE_SIZE_KiB": k["WRITE_SIZE_KiB_avg"],
                             "fetch_factor": cal["fetch_factor"], "factor_from": cal["factor_from"],
                             "structural_bytes": cal.get("structural_bytes"),
                             "revision": d.get("revision")}
            # is the kernel the counters were taken on the kernel of THIS tree?  (sha-256 of its sources, recorded by
            # scripts/profile_round.sh in the same pass - the GPU box has no .git to diff against)
            import hashlib
            recorded, changed = d.get("kernel_sources_sha256") or {}, []
            for rel, digest in recorded.items():
                try:
                    with open(os.path.join(ROOT, rel), "rb") as fsrc:
                        if hashlib.sha256(fsrc.read()).hexdigest() != digest:
                            changed.append(rel)
                except OSError:
                    changed.append(rel)
            out["detail"]["kernel_sources_changed_since_the_pmc_pass"] = (changed if recorded else
                                                                          "unknown (summary older than round 4)")
        else:       # summaries of earlier rounds: the guide's streaming-read factor, uncalibrated for a gather
            out["bytes"] = k["hbm_bytes_per_launch_corrected"]
            out["detail"] = {"note": "2 x FETCH_SIZE (streaming-read correction), not calibrated for this pattern"}
    except Exception as e:
        out["detail"] = {"error": f"{type(e).__name__}: {e}"}
    return out


def cpu_baseline(log2_sample, seed):
    from oracle import c_oracle
    n = 1 << log2_sample
    rng = np.random.default_rng(seed)
    base = np.frombuffer(
        (15112221349535400772501151409588531511454012693041857206046113283949847762202).to_bytes(32, "little")
        + (46316835694926478169428394003475163141307993866256225615783033603165251855960).to_bytes(32, "little")
        + (1).to_bytes(32, "little"), np.uint8)
    # a few distinct generators are enough for timing the per-term ladders
    _, pts_small = c_oracle.fixed_base(base, rand_scalars(rng, 64))
    pts = np.tile(pts_small, (n // 64, 1))
    sc = rand_scalars(rng, n)
    t0 = time.perf_counter()
    c_oracle.vector_commitment(sc, np.zeros(32, np.uint8), pts, pts[0])
    dt = time.perf_counter() - t0
    return {"value": n / dt, "unit": "scalar-mults/s", "cores": 1, "kind": "port",
            "host_cores_available": os.cpu_count(), "host_cores_granted": c_oracle.host_threads(),
            "sample": f"oracle/ed25519_oracle.c vector_commitment (reference algorithm: per-term "
                      f"253-bit double-and-add + product tree), n=2^{log2_sample} uniform scalars, "
                      f"{dt:.1f} s on 1 core"}


def strong_cpu_baseline(log2n, seed):
    """oracle/cpu_pippenger.c: the same commitment by Pippenger (signed windows, 51-bit limbs, 7M mixed additions)
    on every host core - the algorithm class the GPU path uses, so that the GPU/CPU ratio has an honest
    denominator next to the reference algorithm's."""
    from oracle import c_oracle
    n = 1 << log2n
    rng = np.random.default_rng(seed)
    base = np.frombuffer(
        (15112221349535400772501151409588531511454012693041857206046113283949847762202).to_bytes(32, "little")
        + (46316835694926478169428394003475163141307993866256225615783033603165251855960).to_bytes(32, "little")
        + (1).to_bytes(32, "little"), np.uint8)
    _, pts_small = c_oracle.fixed_base(base, rand_scalars(rng, 256))
    pts = np.tile(pts_small, (n // 256, 1))
    sc = rand_scalars(rng, n)
    cores = os.cpu_count() or 1
    out = {"algorithm": "Pippenger, signed windows, one slice per thread (oracle/cpu_pippenger.c)", "n": f"2^{log2n}"}
    for label, threads in (("all_cores", cores), ("one_core", 1)):
        m = n if threads > 1 else n >> 3
        c_oracle.pippenger_msm(sc[:4096], pts[:4096], threads)              # warm the thread pool / caches
        t0 = time.perf_counter()
        c_oracle.pippenger_msm(sc[:m], pts[:m], threads)
        dt = time.perf_counter() - t0
        out[label] = {"threads": threads, "terms": m, "seconds": round(dt, 4), "scalar_mults_per_s": round(m / dt, 1)}
    out["value"] = out["all_cores"]["scalar_mults_per_s"]
    out["cores"] = cores
    return out


def python_reference_baseline(seed, budget_s=40.0):
    """The pure-Python statement of the REFERENCE algorithm (oracle/ac20_ref.vector_commitment: per-term
    right-to-left double-and-add on Python big ints + the reduce tree; the stand-in for the MPyC-based
    reference, which is installable on neither machine), one core, timed at n = 2^10 and - budget
    permitting - 2^12 and 2^14.  The algorithm is exactly linear in n (n independent ladders + n - 1 additions), so
    the rate extrapolates to 2^20; the line says which sizes were measured."""
    import random
    from oracle import ac20_ref as ac
    from oracle import ed25519_ref as ed
    rng = random.Random(seed)
    small = [ed.pt_repeat(ed.BASE, rng.randrange(1, ed.ELL)) for _ in range(16)]
    out = {"algorithm": "per-term 253-bit double-and-add + product tree (pivot.py:143-144), Python big ints",
           "cores": 1, "measured": {}}
    spent = 0.0
    for lg in (10, 12, 14):
        n = 1 << lg
        if lg > 10 and spent * 5.5 > budget_s:     # the next size costs ~4x everything measured so far
            break
        g = [small[i % 16] for i in range(n)]
        x = [rng.randrange(ed.ELL) for _ in range(n)]
        t0 = time.perf_counter()
        ac.vector_commitment(x, rng.randrange(ed.ELL), g, ed.BASE, signed_exponents=False)
        dt = time.perf_counter() - t0
        spent += dt
        out["measured"][f"n2^{lg}"] = {"seconds": round(dt, 3), "scalar_mults_per_s": round(n / dt, 1)}
    best = max(v["scalar_mults_per_s"] for v in out["measured"].values())
    out["scalar_mults_per_s"] = best
    out["extrapolated_seconds_n2^20"] = round((1 << 20) / best, 1)
    out["note"] = "2^20 figure extrapolated linearly from the measured sizes (not run: ~" \
                  f"{(1 << 20) / best / 60:.0f} min per commitment)"
    return out


def prove_timing(vm, ctx, n_pow, rng):
    """AC20 Protocol 5 prove at N = 2^n_pow, device-resident inputs, both transcripts."""
    N = 1 << n_pow
    n = N - 1
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    out = {}
    exps = vm.ScalarVector.from_array(rand_scalars(rng, n))
    t0 = time.perf_counter()
    g = vm.PointVector.fixed_base(group.generator, exps, keep_proj=True)
    ctx.sync()
    out["create_generators_ms"] = (time.perf_counter() - t0) * 1e3
    gens = {"g": g, "h": group.generator, "k": vm.Ed25519Point.repeat(group.generator, 0x1234567)}
    t0 = time.perf_counter()
    g.precompute([gens["h"], gens["k"]], wide=True)     # CRS setup, as circuit_sat.create_generators does
    ctx.sync()
    out["crs_table_ms"] = (time.perf_counter() - t0) * 1e3
    x = vm.ScalarVector.from_array(rand_scalars(rng, n))
    L = vm.pivot.LinearForm(vm.ScalarVector.from_array(rand_scalars(rng, n)))
    gamma = 0x7654321
    y = gf(L(x))
    P = vm.pivot.vector_commitment(x, gamma, g, gens["h"])
    for mode in ("compact", "reference"):
        if mode == "compact":
            vm.compressed_pivot.generators_digest(gens)      # CRS digest is setup, cached
        runs, inside = [], []
        for attempt in range(4):                 # the first call grows the stream workspaces; then 3 timed
            r = vm.ScalarVector.from_array(rand_scalars(rng, n))
            ctx.sync()
            vm.pivot.hash_stats(reset=True)
            t0 = time.perf_counter()
            proof = vm.compressed_pivot.protocol_5_prover(gens, P, L, y, x, gamma, gf, transcript=mode,
                                                          r=r, rho=0x1111)
            ctx.sync()
            runs.append((time.perf_counter() - t0) * 1e3)
            prove_hash = vm.pivot.hash_stats()
            inside.append(prove_hash["seconds"] * 1e3)
        vm.pivot.hash_stats(reset=True)
        out[f"prove_ms_{mode}_first_call"] = runs[0]
        out[f"prove_ms_{mode}"] = sorted(runs[1:])[1]            # median of the three steady runs
        out[f"prove_ms_{mode}_min"] = min(runs[1:])
        # (what the build controls: the time OUTSIDE sha256.update, run by run - the host's hashing speed itself wanders
        # by several per cent between runs on a shared box)
        outside_p = sorted(t - h for t, h in zip(runs[1:], inside[1:]))
        vruns, vinside = [], []
        for attempt in range(4):                 # the first call creates contexts and buffers; then 3 timed
            vm.pivot.hash_stats(reset=True)
            t0 = time.perf_counter()
            ok = vm.compressed_pivot.protocol_5_verifier(gens, P, L, y, proof, gf, transcript=mode)
            vruns.append((time.perf_counter() - t0) * 1e3)
            vinside.append(vm.pivot.hash_stats()["seconds"] * 1e3)
            assert ok is True
        outside_v = sorted(t - h for t, h in zip(vruns[1:], vinside[1:]))
        out[f"verify_ms_{mode}_first_call"] = vruns[0]
        out[f"verify_ms_{mode}"] = sorted(vruns[1:])[1]          # median of the three steady runs
        out[f"verify_ms_{mode}_min"] = min(vruns[1:])
        if mode == "reference":
            # The floor of the reference's transcript: one sequential SHA-256 over the decimal text of every round's
            # generators and form (pivot.py:131-136) on ONE host core.  Measured, not asserted: the same number of
            # bytes through hashlib alone (64-MiB pieces of a resident buffer), and the time the prover itself spent
            # inside update().
            import hashlib
            nbytes = prove_hash["bytes"]
            buf = np.random.default_rng(1).integers(48, 58, size=min(nbytes, 64 << 20), dtype=np.uint8)   # digits
            floors = []
            for _ in range(3):
                h = hashlib.sha256()
                t0 = time.perf_counter()
                left = nbytes
                while left > 0:
                    h.update(memoryview(buf)[:min(left, len(buf))])
                    left -= len(buf)
                h.digest()
                floors.append((time.perf_counter() - t0) * 1e3)
            floor = min(floors)
            vh = vm.pivot.hash_stats(reset=True)
            out["hash_floor"] = {
                "bytes_hashed_per_prove": nbytes, "hash_floor_ms": round(floor, 2),
                "host_sha256_GBps": round(nbytes / floor / 1e6, 3),
                "prove_ms_inside_sha256_update": round(inside[-1], 2),
                "prove_ms_outside_sha256_update": round(outside_p[1], 2),
                "verify_ms_outside_sha256_update": round(outside_v[1], 2),
                "prove_floor_plus_outside_over_floor": round((floor + outside_p[1]) / floor, 4),
                "verify_floor_plus_outside_over_floor": round((floor + outside_v[1]) / floor, 4),
                "prove_over_floor": round(out["prove_ms_reference"] / floor, 4),
                "verify_bytes_hashed": vh["bytes"],
                "verify_over_floor": round(out["verify_ms_reference"] / (floor * vh["bytes"] / max(nbytes, 1)), 4),
                # (the host's hashing speed wanders by several per cent between runs on a shared box: the ratios above
                # are median run over best floor; these are best run over best floor)
                "prove_over_floor_best_run": round(out["prove_ms_reference_min"] / floor, 4),
                "verify_over_floor_best_run": round(out["verify_ms_reference_min"] /
                                                    (floor * vh["bytes"] / max(nbytes, 1)), 4),
                "what": "floor = hashlib.sha256 alone over the same number of bytes on one host core (best of 3); "
                        "the reference's transcript format makes this sequential hash inherent (pivot.py:131-136)"}
        # a Protocol-5 prove moves ~768 * N algorithmic bytes (two N-term commitments + per round
        # two half-size commitments, the fold and the scalar folds); Fiat-Shamir text excluded
        alg = 768 * N
        ms = out[f"prove_ms_{mode}"]
        out[f"roofline_{mode}"] = {
            "bound": "hbm", "algorithmic_bytes": alg, "achieved_GBps": alg / (ms * 1e-3) / 1e9,
            "peak_GBps": HBM_PEAK_GBPS, "frac": alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
            "dominant": ("k_msm_bucket (the announcement and 5 rounds of two N-term table commitments) and k_fold_jump "
                         "(those 5 rounds' generator folds in one pass); the other 14 rounds run on the folded "
                         "vector's table (profiles/*_prove_compact_kernel_stats.csv)"
                         if mode == "compact" else
                         "host SHA-256 of ~1 GB of decimal pre-image text on one core (~85 % of the wall time); on "
                         "the GPU k_fold, the exact replay of (g_l ** c) * g_r "
                         "(profiles/*_prove_reference_kernel_stats.csv)"),
            "transcript": ("build-defined compact byte transcript: NOT the reference's challenges" if mode == "compact"
                           else "the reference's str(input_list) transcript, byte formats as recalled from MPyC ([mpyc-recall]): "
                                "proofs bit-identical to the reference's own modules run over the build-written MPyC "
                                "stand-in (tests/golden/mpyc_shim), not to a run over real MPyC "
                                "(scripts/check_against_mpyc.py pins that on a machine that has it)")}
    return out


def bn256_timing(vm, ctx, n_pow):
    """BASELINE config 5: BN-256 G1 / twist sums of 2^n_pow terms (the Pinocchio prover's MSMs),
    variable-base and over a prepared (tabulated) key vector; affine outputs.  Timing inputs: the
    generator repeated with uniform scalars (parity is tests/test_gpu_bn256.py)."""
    n = 1 << n_pow
    p_mod = 65000549695646603732796438742359905742825358107623003571877145026864184071783
    g1 = (1).to_bytes(32, "little") + (p_mod - 2).to_bytes(32, "little")
    g2 = b"".join(v.to_bytes(32, "little") for v in (
        64746500191241794695844075326670126197795977525365406531717464316923369116492,
        21167961636542580255011770066570541300993051739349375019639421053990175267184,
        17778617556404439934652658462602675281523610326338642107814333856843981424549,
        20666913350058776956210519119118544732556678129809273996262322366050359951122))
    rng = np.random.default_rng(7)
    out = {}
    order = 65000549695646603732796438742359905742570406053903786389881062969044166799969
    for group, gen, width, tag in ((1, g1, 64, "g1"), (2, g2, 128, "g2")):
        sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        sc[:, 31] &= 0x7F
        # DISTINCT points e_i * G (vmpc_bn256_fixed_base_dev): with one point repeated every bucket sum would
        # run the doubling branch of the incomplete addition law, which no real key vector does
        ex = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        ex[:, 31] &= 0x7F
        dg, de = ctx.upload(np.frombuffer(gen, np.uint8)), ctx.upload(ex)
        dp, ds, res = ctx.alloc(width * n), ctx.upload(sc), ctx.alloc(width)
        t0 = time.perf_counter()
        ctx.bn256_fixed_base(group, dg.ptr, de.ptr, n, dp.ptr)
        ctx.sync()
        out[f"{tag}_key_setup_ms"] = (time.perf_counter() - t0) * 1e3
        table = ctx.bn256_table_build(group, dp.ptr, n)
        for name, fn in (("variable_base", lambda: ctx.bn256_msm(group, ds.ptr, dp.ptr, n, res.ptr)),
                         ("prepared_key", lambda: ctx.bn256_table_msm(group, table.ptr, n, ds.ptr, n, res.ptr, None))):
            fn()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            ctx.sync()
            out[f"{tag}_{name}_ms"] = (time.perf_counter() - t0) / 3 * 1e3
            # size-independent property at full size: sum s_i (e_i G) == (sum s_i e_i mod n) G
            if name == "variable_base":
                tot = sum(int.from_bytes(bytes(a), "little") * int.from_bytes(bytes(b), "little")
                          for a, b in zip(sc, ex)) % order
                dt_, want = ctx.upload(np.frombuffer(tot.to_bytes(32, "little"), np.uint8)), ctx.alloc(width)
                ctx.bn256_fixed_base(group, dg.ptr, dt_.ptr, 1, want.ptr)
                var_result = ctx.download(res.ptr, width).tobytes()
                assert var_result == ctx.download(want.ptr, width).tobytes(), f"BN-256 {tag} MSM property check failed"
            else:
                assert ctx.download(res.ptr, width).tobytes() == var_result, f"BN-256 {tag} table MSM differs"
        # what pynocchio.PreparedKey asks for: the sum in Jacobian coordinates (the affine conversion's inversion chain
        # is a single-lane job the host does in microseconds)
        jac = ctx.alloc(3 * width // 2)
        ctx.bn256_table_msm(group, table.ptr, n, ds.ptr, n, None, jac.ptr)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(3):
            ctx.bn256_table_msm(group, table.ptr, n, ds.ptr, n, None, jac.ptr)
        ctx.sync()
        out[f"{tag}_prepared_key_jacobian_out_ms"] = (time.perf_counter() - t0) / 3 * 1e3
        # the bucket pass of the prepared-key sum alone, against the integer-ALU ceiling of ITS inner operation
        # (Jacobian mixed addition on the Montgomery-form field, madd-2007-bl: 7M + 4S; G2 over F_p^2), measured
        # in this run by a register-resident chain on every lane (vmpc_bn256_madd_rate)
        ctx.profile(True)
        ctx.profile_read(reset=True)
        for _ in range(3):
            ctx.bn256_table_msm(group, table.ptr, n, ds.ptr, n, res.ptr, None)
        stages = {k: ms / max(c, 1) for k, (ms, c) in ctx.profile_read(reset=True).items()}
        ctx.profile(False)
        windows = 17                                     # 256-bit scalars in signed 16-bit digits
        peak = max(ctx.bn256_madd_rate(group, 100) for _ in range(2))
        bucket_s = stages.get("bn_bucket", 0.0) / 1e3
        out[f"{tag}_stages_us"] = {k: round(v * 1e3, 1) for k, v in stages.items() if v > 0}
        out[f"{tag}_alu"] = {"unit": "G mixed-additions/s", "peak": peak / 1e9,
                             "peak_source": "vmpc_bn256_madd_rate: register-resident Jacobian mixed additions on "
                                            "every lane, measured in this run",
                             "mixed_additions_per_launch": n * windows,
                             "kernel": "gk_bucket (stage bn_bucket)", "kernel_ms": bucket_s * 1e3,
                             "achieved": n * windows / bucket_s / 1e9 if bucket_s else None,
                             "frac": n * windows / bucket_s / peak if bucket_s else None,
                             "whole_sum_frac": n * windows / (out[f"{tag}_prepared_key_ms"] * 1e-3) / peak,
                             # what pynocchio.PreparedKey actually asks for: the sum left in Jacobian coordinates (one
                             # host inversion instead of a ~380-multiplication single-lane chain on the device)
                             "whole_sum_frac_jacobian_out":
                                 n * windows / (out[f"{tag}_prepared_key_jacobian_out_ms"] * 1e-3) / peak}
        # algorithmic bytes per term: 32-byte scalar + affine point (64 B G1, 128 B twist)
        per_term = 32 + width
        out[f"{tag}_roofline"] = {"bound": "hbm", "algorithmic_bytes_per_term": per_term,
                                  "achieved_GBps_prepared_key": per_term * n / (out[f"{tag}_prepared_key_ms"] * 1e-3) / 1e9,
                                  "peak_GBps": HBM_PEAK_GBPS}
        out[f"{tag}_roofline"]["frac"] = out[f"{tag}_roofline"]["achieved_GBps_prepared_key"] / HBM_PEAK_GBPS
        del table
    return out


def other_sizes_timing(vm, ctx, pows):
    """One variable-base commitment alone at the other BASELINE sizes: config 2 (2^16), one GPU's share
    of config 4 (2^21 of 2^24 over 8 GPUs) and 2^24 on a single GPU."""
    group = vm.EllipticCurve("Ed25519", "projective")
    rng = np.random.default_rng(11)
    out = {}
    for lg in pows:
        n = 1 << lg
        pts = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(rand_scalars(rng, n)),
                                        keep_proj=False)
        sc = vm.ScalarVector.from_array(rand_scalars(rng, n))
        res = ctx.alloc(128)
        ctx.msm(sc.ptr, pts.affine_ptr, n, None, None, 0, res.ptr, None)
        ctx.sync()
        reps = 10 if lg <= 21 else 3
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.msm(sc.ptr, pts.affine_ptr, n, None, None, 0, res.ptr, None)
        ctx.sync()
        dt = (time.perf_counter() - t0) / reps
        out[f"n2^{lg}"] = {"ms": round(dt * 1e3, 3), "M_scalar_mults_per_s": round(n / dt / 1e6, 1)}
        # the same commitment over the generators as circuit_sat.create_generators hands them to vector_commitment:
        # a fixed-base table, rows as pivot._auto_tabulate picks them (16 rows below 2^19 generators, the 13-row
        # wide-window table from there up to 2^22, then whatever fits 1 GiB) - the latency a commitment actually pays
        tab = vm.PointVector(pts.a, None, ctx).precompute([], rows=vm.pivot._auto_table_rows(n)[0])
        t_ = tab._table
        for _ in range(2):
            ctx.msm_table(t_.ptr, t_.n, 0, sc.ptr, n, None, res.ptr, None, rows=t_.rows)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.msm_table(t_.ptr, t_.n, 0, sc.ptr, n, None, res.ptr, None, rows=t_.rows)
            ctx.sync()
        dt = (time.perf_counter() - t0) / reps
        out[f"n2^{lg}"].update({"crs_table_rows": t_.rows, "ms_over_crs_table": round(dt * 1e3, 3),
                                "M_scalar_mults_per_s_over_crs_table": round(n / dt / 1e6, 1)})
        del tab, t_
        del pts, sc
    return out


def commitment_scalars(rng, n):
    """The distribution of the committed vector [z] that SURVEY.md section 8d measured on the demo circuit
    (circuit_sat_cb.py:91-103: inputs, gadget witnesses, zero pads, then polynomial evaluations): 54 % zeros, 9 % in
    {1, 2}, 37 % uniform field elements.  (n, 32) uint8 little-endian, positions shuffled."""
    a = rand_scalars(rng, n)
    kind = rng.random(n)
    a[kind < 0.54] = 0
    small = (kind >= 0.54) & (kind < 0.63)
    a[small] = 0
    a[small, 0] = rng.integers(1, 3, size=int(small.sum()), dtype=np.uint8)
    return a


def distribution_timing(vm, ctx, pows):
    """Uniform scalars beside the commitment distribution of [z] (zero / one / two buckets hold most of the terms: the
    tiled sort and the split-bucket path of csrc/msm_sort.hip, msm.hip), at config 2's and the headline's size: one
    commitment alone (host synchronises after each), back to back on one stream, and K per pass over the CRS table
    (vmpc_msm_table_batch_dev).  Results are checked by the exponent identity against the product's fixed-base kernel."""
    group = vm.EllipticCurve("Ed25519", "projective")
    rng = np.random.default_rng(20200152)
    out = {}
    order = vm.groups.ORDER
    for lg in pows:
        n = 1 << lg
        exps = rand_scalars(rng, n)
        pts = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps), keep_proj=False)
        tab = vm.PointVector(pts.a, None, ctx).precompute([], rows=vm.pivot._auto_table_rows(n)[0])   # (as _auto_tabulate)
        t_ = tab._table
        res = ctx.alloc(128)
        entry = {"crs_table_rows": t_.rows}
        reps = 20 if lg <= 16 else 10
        for name, arr in (("uniform", rand_scalars(rng, n)), ("commitment_distribution", commitment_scalars(rng, n))):
            sc = vm.ScalarVector.from_array(arr)
            forms = {"prepared_per_call": lambda: ctx.msm(sc.ptr, pts.affine_ptr, n, None, None, 0, res.ptr, None),
                     "over_crs_table": lambda: ctx.msm_table(t_.ptr, t_.n, 0, sc.ptr, n, None, res.ptr, None, rows=t_.rows)}
            e = {}
            want = None
            for form, fn in forms.items():
                for _ in range(2):
                    fn()
                ctx.sync()
                got = vm.Ed25519Point.from_proj_bytes(ctx.download(res.ptr, 128).tobytes()[:96]).normalize()
                if want is None:
                    tot = exponent_sum(arr, exps, order)
                    want = vm.PointVector.fixed_base(group.generator, [tot], keep_proj=False)[0]
                assert got == want, f"MSM property check failed ({name}, {form}, n=2^{lg})"
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                    ctx.sync()
                alone = (time.perf_counter() - t0) / reps
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                ctx.sync()
                b2b = (time.perf_counter() - t0) / reps
                e[form] = {"alone_ms": round(alone * 1e3, 4), "back_to_back_ms": round(b2b * 1e3, 4),
                           "M_scalar_mults_per_s_back_to_back": round(n / b2b / 1e6, 1)}
            e["nonzero_fraction"] = round(float((arr != 0).any(axis=1).mean()), 4)
            entry[name] = e
            del sc
        for form in ("prepared_per_call", "over_crs_table"):
            entry[f"commitment_over_uniform_{form}_alone"] = round(
                entry["commitment_distribution"][form]["alone_ms"] / entry["uniform"][form]["alone_ms"], 3)
        # K commitments per pass over the table (distinct uniform scalar vectors): the sort is per vector, the bucket
        # reduction and the window recombination are paid once per pass
        per_pass = {}
        for K in (2, 4, 8):
            vecs = [vm.ScalarVector.from_array(rand_scalars(rng, n)) for _ in range(K)]
            outk = ctx.alloc(128 * K)
            try:
                for _ in range(2):
                    ctx.msm_table_batch(t_.ptr, t_.n, 0, [v.ptr for v in vecs], n, None, outk.ptr, None, rows=t_.rows)
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(reps):
                    ctx.msm_table_batch(t_.ptr, t_.n, 0, [v.ptr for v in vecs], n, None, outk.ptr, None, rows=t_.rows)
                ctx.sync()
                dt = (time.perf_counter() - t0) / reps
                per_pass[f"K{K}"] = {"ms_per_pass": round(dt * 1e3, 4), "ms_per_commitment": round(dt / K * 1e3, 4),
                                     "M_scalar_mults_per_s": round(K * n / dt / 1e6, 1)}
            except Exception as ex:
                per_pass[f"K{K}"] = {"error": f"{type(ex).__name__}: {ex}"}
            del vecs, outk
        entry["commitments_per_pass_over_crs_table"] = per_pass
        out[f"n2^{lg}"] = entry
        del tab, t_, pts
    out["checked"] = "exponent identity against the product's fixed-base kernel, every (distribution, form)"
    return out


def clocks_sample():
    """one reading of the GPU's clocks and power cap (rocm-smi), so that box-to-box spread of the headline has
    something to be read against; best effort.  Taken FIRST, before this process touches the GPU (a child started
    later would be a program exec'd from a GPU-initialised process), and not at all under a profiler's preload
    (rocprofv3 initialises the GPU inside every process it is preloaded into, the child included)."""
    import shutil
    import subprocess
    if any("rocprof" in os.environ.get(k, "").lower() for k in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB")):
        return {"skipped": "running under a profiler preload"}
    exe = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    out = {}
    try:
        txt = subprocess.run([exe, "-d", "0", "--showclocks", "--showmaxpower", "--showpower", "--showperflevel"],
                             capture_output=True, text=True, timeout=20).stdout
        for line in txt.splitlines():
            # "GPU[0]\t\t: sclk clock level: 1: (2400Mhz)" / "GPU[0]\t\t: Max Graphics Package Power (W): 1400.0"
            parts = [p_.strip() for p_ in line.split(":")]
            if len(parts) < 3 or not parts[0].startswith("GPU["):
                continue
            low = parts[1].lower()
            if any(w in low for w in ("sclk", "mclk", "fclk", "power", "performance level")):
                out[parts[1][:60]] = ": ".join(parts[2:])
    except Exception as e:
        out["error"] = f"{type(e).__name__}: {e}"
    return out


_SAMPLER_CODE = r"""
import glob, json, os, sys, time
# runs as a CHILD started before the parent touches the GPU; reads sysfs only (no HIP, no rocm-smi library).  Every card
# is sampled, keyed by its PCI address: which one the parent computes on is only known after it has initialised the GPU.
cards = {}
for p in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
    dev = os.path.realpath(p.rsplit("/", 1)[0])
    power = sorted(glob.glob(dev + "/hwmon/hwmon*/power1_average")) + sorted(glob.glob(dev + "/hwmon/hwmon*/power1_input"))
    cards[os.path.basename(dev)] = (dev, power[0] if power else None)
def cur_mhz(p):
    try:
        for line in open(p):
            if "*" in line:
                return float(line.split(":")[1].strip().lower().split("m")[0])
    except Exception:
        return None
while True:
    rec = {"t": time.time(), "cards": {}}
    for pci, (dev, power) in cards.items():
        c = {"sclk": cur_mhz(dev + "/pp_dpm_sclk"), "mclk": cur_mhz(dev + "/pp_dpm_mclk")}
        if power:
            try:
                c["w"] = int(open(power).read()) / 1e6
            except Exception:
                pass
        rec["cards"][pci] = c
    sys.stdout.write(json.dumps(rec) + "\n")
    sys.stdout.flush()
    time.sleep(0.003)
"""


class ClockSampler:
    """sclk / mclk / socket power read from sysfs every few ms by a child process that is started BEFORE this process
    initialises the GPU (a child started later would be an exec from a GPU-initialised process, which the pool's boxes
    refuse); window(t0, t1) summarises the samples taken while a measured loop ran - the clocks the kernels actually
    saw, next to the idle reading of clocks_sample()."""

    def __init__(self):
        import subprocess
        import threading
        self.samples, self.proc = [], None
        if any("rocprof" in os.environ.get(k, "").lower() for k in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB")):
            return                                   # (a profiler's preload initialises the GPU in every child)
        try:
            self.proc = subprocess.Popen([sys.executable, "-c", _SAMPLER_CODE], stdout=subprocess.PIPE,
                                         stderr=subprocess.DEVNULL, text=True)
        except Exception:
            self.proc = None
            return

        def pump():
            for line in self.proc.stdout:
                try:
                    self.samples.append(json.loads(line))
                except Exception:
                    pass
        threading.Thread(target=pump, daemon=True).start()

    def window(self, t0, t1, pci=None):
        """min / median / max over the samples of card `pci` (its PCI address, e.g. "0000:05:00.0"; None: the only
        card, else nothing) taken between the two time.time() stamps"""
        inside = [r for r in self.samples if t0 <= r["t"] <= t1]
        out = {"samples": len(inside), "window_ms": round((t1 - t0) * 1e3, 1), "card": pci}
        names = sorted({k for r in inside for k in r.get("cards", {})})
        if pci is None and len(names) == 1:
            pci = out["card"] = names[0]
        if pci not in names:
            out["cards_seen"] = names
            return out
        for key, name in (("sclk", "sclk_mhz"), ("mclk", "mclk_mhz"), ("w", "socket_power_w")):
            vals = sorted(r["cards"][pci][key] for r in inside if r.get("cards", {}).get(pci, {}).get(key) is not None)
            if vals:
                out[name] = {"min": vals[0], "median": vals[len(vals) // 2], "max": vals[-1]}
        return out

    def stop(self):
        if self.proc is not None:
            try:
                self.proc.kill()                     # the exact child started above
                self.proc.wait(timeout=5)
            except Exception:
                pass
            self.proc = None


def pinocchio_timing(vm, ctx, n_pow):
    """BASELINE config 5 as ONE number: pynocchio.compute_proof (trinocchio/pynocchio.py:229-246 of the reference -
    seven G1 sums and one twist sum over the evaluation key, c and h shared between them) over a prepared key of 2^n_pow
    terms, scalars handed over as (n, 32) arrays.  Synthetic key (every entry the generator): timing only - parity of
    compute_proof is tests/test_gpu_bn256.py::test_compute_proof_matches_reference_fixture."""
    from verifiable_mpc_amd import pynocchio as pn
    n = 1 << n_pow
    rng = np.random.default_rng(3)
    key = pn.PreparedKey.synthetic(ctx, n)

    class Delta:
        v, w, y = 11, 22, 33
    c = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    c[:, 31] &= 0x7F
    h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    h[:, 31] &= 0x7F
    first = pn.compute_proof(None, c, h, key, Delta)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        proof = pn.compute_proof(None, c, h, key, Delta)
        times.append((time.perf_counter() - t0) * 1e3)
    assert proof == first
    # the six G1 sums over c_mid alone: ONE multi-key pass (vmpc_bn256_table_msm_multi_dev), Jacobian out
    g1 = [key.vectors[name] for name in pn._SHARED_G1]
    dc, outm = ctx.upload(c), ctx.alloc(96 * len(g1))
    for _ in range(2):
        ctx.bn256_table_msm_multi(1, [v.table.ptr for v in g1], g1[0].n, dc.ptr, n, outm.ptr)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(5):
        ctx.bn256_table_msm_multi(1, [v.table.ptr for v in g1], g1[0].n, dc.ptr, n, outm.ptr)
    ctx.sync()
    multi_ms = (time.perf_counter() - t0) / 5 * 1e3
    # ... and each of them equals the single-key pass over the same table
    one = ctx.alloc(96)
    ctx.bn256_table_msm(1, g1[2].table.ptr, g1[2].n, dc.ptr, n, None, one.ptr)
    ctx.sync()
    same = pn._from_jacobian(1, ctx.download(one.ptr, 96).tobytes()) == \
        pn._from_jacobian(1, ctx.download(outm.ptr + 96 * 2, 96).tobytes())
    assert same, "multi-key pass differs from the single-key pass"
    peak = max(ctx.bn256_madd_rate(1, 100) for _ in range(2))
    return {"whole_proof_ms": round(sorted(times)[len(times) // 2], 3), "whole_proof_ms_min": round(min(times), 3),
            "terms_per_sum": n, "sums": "7 x G1 + 1 x G2 (pynocchio.compute_proof over a PreparedKey: the six G1 sums "
                                        "over c_mid as one multi-key pass)",
            "g1_six_sums_one_pass_ms": round(multi_ms, 3), "g1_ms_per_sum_in_one_pass": round(multi_ms / len(g1), 3),
            "g1_whole_sum_frac_jacobian_out_in_one_pass": round(len(g1) * n * 17 / (multi_ms * 1e-3) / peak, 3),
            "key": "synthetic: distinct multiples of the generator, prepared (tabulated) once, untimed"}


def sharded_prove_timing(vm, ctx, n_pow, world, rank, dist, torch, comm=None):
    """AC20 Protocol 5 (compact transcript) with g_hat in `world` blocks, one per rank
    (verifiable_mpc_amd/sharded.py): one exchange of two 128-byte points per rank and round.  With `comm` the
    rounds run inside the C library's sharded round context (vmpc_p4_create_sharded)."""
    from verifiable_mpc_amd import sharded
    N = 1 << n_pow
    n = N - 1
    group = vm.EllipticCurve("Ed25519", "projective")
    gf = vm.GF(group.order)
    rng = np.random.default_rng(4242)                      # the same inputs on every rank
    exps = rand_scalars(rng, n)
    exps[:, 0] |= 1
    h, k = group.generator, vm.Ed25519Point.repeat(group.generator, 0x1234567)
    t0 = time.perf_counter()
    crs = sharded.ShardedCrs.from_exponents(h, k, exps, world, [rank], dist, torch, ctx, comm=comm)
    crs.digest()
    ctx.sync()
    out = {"crs_block_ms": (time.perf_counter() - t0) * 1e3}
    x = vm.ScalarVector.from_array(rand_scalars(rng, n))
    L = vm.pivot.LinearForm(vm.ScalarVector.from_array(rand_scalars(rng, n)))
    gamma = 0x7654321
    y = gf(L(x))
    P = crs.commit([(x.concat([gamma]), None)])[0]
    out["blocks"] = world
    out["rounds_in"] = "libvmpc_hip (vmpc_p4_create_sharded)" if comm is not None else "python (sharded.py)"
    out["transport"] = comm.kind if comm is not None else "torch.distributed"
    runs = []
    for attempt in range(4):
        r = vm.ScalarVector.from_array(rand_scalars(rng, n))
        ctx.sync()
        dist.barrier()
        t0 = time.perf_counter()
        proof = sharded.protocol_5_prover(crs, P, L, y, x, gamma, gf, r, 0x1111)
        ctx.sync()
        dist.barrier()
        runs.append((time.perf_counter() - t0) * 1e3)
    out["prove_ms_compact_first_call"] = runs[0]
    out["prove_ms_compact"] = sorted(runs[1:])[1]
    out["prove_ms_compact_min"] = min(runs[1:])
    mine = b"".join(proof[key].to_affine_bytes() for key in sorted(proof) if key[0] in "AB")
    every = [None] * world
    dist.all_gather_object(every, mine)
    assert all(e == mine for e in every), "ranks disagree on the proof"
    out["ranks_agree"] = True
    if rank == 0:
        # the sharded proof is an ordinary compact proof: the single-GPU verifier accepts it over the whole CRS
        g = vm.PointVector.fixed_base(h, vm.ScalarVector.from_array(exps), keep_proj=False)
        ok = vm.compressed_pivot.protocol_5_verifier({"g": g, "h": h, "k": k}, P, L, y, proof, gf, transcript="compact")
        assert ok is True, "the unsharded verifier rejects the sharded proof"
        out["verified"] = True
    if rank == 0 and world == 1:
        # one rank: the same proof by the unsharded prover, same process, same box - what the exchange and the
        # sharded entry point cost (g is already here for the verification)
        g.precompute([h, k])
        gens = {"g": g, "h": h, "k": k}
        vm.compressed_pivot.generators_digest(gens)
        plain = []
        for attempt in range(4):
            r = vm.ScalarVector.from_array(rand_scalars(rng, n))
            ctx.sync()
            t0 = time.perf_counter()
            vm.compressed_pivot.protocol_5_prover(gens, P, L, y, x, gamma, gf, transcript="compact", r=r, rho=0x1111)
            ctx.sync()
            plain.append((time.perf_counter() - t0) * 1e3)
        out["unsharded_prove_ms_compact"] = sorted(plain[1:])[1]
        out["sharded_over_unsharded"] = out["prove_ms_compact"] / out["unsharded_prove_ms_compact"]
    out["rounds"] = n_pow - 1
    return out


def config4_timing(vm, parallel, shard, total_log2, world, rank, dist, barrier, torch):
    """BASELINE config 4 as stated: ONE commitment of 2^total_log2 terms (2^24), cyclic shards of 2^total_log2 / world
    terms per rank (2^21 at 8 ranks), one exchange of a 128-byte point per rank + rank-ordered add (SURVEY.md 8e,
    pivot.py:143-144).  Timed one commitment at a time (barrier + device synchronisation on both sides, max over
    ranks) and checked by the cross-rank exponent identity  sum_i s_i (e_i B) == (sum_i s_i e_i mod l) B."""
    n4 = (1 << total_log2) // world
    assert n4 >= 8 and n4 * world == 1 << total_log2, "config 4 needs a power-of-two world size"
    group = vm.EllipticCurve("Ed25519", "projective")
    rng = np.random.default_rng(20200152 + 4 + 1000 * rank)
    exps_arr, sc_arr = rand_scalars(rng, n4), rand_scalars(rng, n4)
    pts = vm.PointVector.fixed_base(group.generator, vm.ScalarVector.from_array(exps_arr), keep_proj=False)
    prepared = vm.PointVector(pts.a, None, shard.backend.ctxs[0]).precompute([], rows=1)
    # ... and as the table pivot._auto_tabulate builds for a shard of this size (2^21 terms per rank at 8 ranks: the
    # 13-row wide-window table, 3.3 GB per rank)
    table_rows = vm.pivot._auto_table_rows(n4)[0]
    tabulated = vm.PointVector(pts.a, None, shard.backend.ctxs[0]).precompute([], rows=table_rows)
    sc = vm.ScalarVector.from_array(sc_arr)
    out = {"total_terms": 1 << total_log2, "terms_per_gpu": n4, "n_gpus": world, "sharding": "cyclic by index",
           "generators": f"resident as a {table_rows}-row table (crs_table), in prepared form (prepared), plain points "
                         f"(variable_base)", "crs_table_rows": table_rows}
    times = {}
    for label, p_ in (("crs_table", tabulated), ("prepared", prepared), ("variable_base", pts)):
        res = shard.commit(sc, p_)                       # grows the workspace; the result that gets checked
        runs = []
        for _ in range(5):
            torch.cuda.synchronize()
            barrier()
            t0 = time.perf_counter()
            got = shard.commit(sc, p_)
            torch.cuda.synchronize()
            barrier()
            runs.append(time.perf_counter() - t0)
            assert got == res, "config 4: the commitment is not reproducible"
        dt = sorted(runs)[len(runs) // 2]
        if dist:
            t = torch.tensor([dt], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        times[label] = (dt, res)
        out[f"ms_per_commitment_{label}"] = round(dt * 1e3, 4)
        out[f"scalar_mults_per_s_{label}"] = round((1 << total_log2) / dt, 1)
    mine = exponent_sum(sc_arr, exps_arr, vm.groups.ORDER)
    if dist:
        every = [None] * world
        dist.all_gather_object(every, mine)
        tot = sum(every) % vm.groups.ORDER
    else:
        tot = mine
    want = vm.PointVector.fixed_base(group.generator, [tot], keep_proj=False)[0]
    for label, (_, res) in times.items():
        assert res == want, f"config 4 ({label}): exponent identity failed on rank {rank}"
    out["checked"] = True
    out["check"] = "cross-rank exponent identity: sum_i s_i (e_i B) == (sum over all ranks of s_i e_i mod l) B"
    return out


def run_steps(shard, k, scalar_vectors, pts, depth, batch):
    """k commitments, in launches of up to `batch` (prepared generators only) with up to `depth` launches in
    flight; every result is fetched to the host, oldest launch first, and its slot refilled at once (with a
    collective every rank must launch and finish in the same order anyway).  The
    commitments of one launch are over DISTINCT scalar vectors (scalar_vectors[0 .. b-1]); single launches cycle
    through the vectors.  Returns (results of the last launch, indices into scalar_vectors they belong to)."""
    per = batch if getattr(pts, "_table", None) is not None else 1
    nvec = len(scalar_vectors)
    backend = getattr(shard, "backend", None)
    if hasattr(backend, "pipelined"):
        backend.pipelined = depth > 1          # phase pipelining over a shared bucket stream (parallel.HipBackend)
    try:
        return _run_steps(shard, k, scalar_vectors, pts, depth, per, nvec)
    finally:
        if hasattr(backend, "pipelined"):
            backend.pipelined = False


def _run_steps(shard, k, scalar_vectors, pts, depth, per, nvec):
    busy, order, size, which, launched, done, last = {}, {}, {}, {}, 0, 0, None
    trace = [] if os.environ.get("VMPC_BENCH_TRACE") else None
    t_prev = time.perf_counter()
    while done < k:
        while launched < k and len(busy) < depth:
            slot = next(s_ for s_ in range(depth) if s_ not in busy)
            b = min(per, k - launched, nvec)
            idx = list(range(b)) if per > 1 else [launched % nvec]
            t_l = time.perf_counter()
            busy[slot] = shard.launch([scalar_vectors[i] for i in idx] if per > 1 else scalar_vectors[idx[0]], pts, slot)
            if trace is not None:
                trace.append(("launch", slot, b, round((time.perf_counter() - t_l) * 1e3, 3)))
            order[slot], size[slot], which[slot] = launched, b, idx
            launched += b
        # Oldest launch first, always.  With a collective every rank must enter the all-gathers in the same
        # order; without one the oldest launch is the one that completes first anyway.  (Completion used to be
        # polled with hipStreamQuery; on this stack a stream query issued while timing events are being
        # recorded costs ONE ~50 ms stall per process around the 250th event - scripts/loop_probe2.py -
        # which landed in the timed region of some step counts.)
        ready = [min(busy, key=lambda s_: order[s_])]
        for s_ in ready:
            t_f = time.perf_counter()
            res = shard.finish(busy.pop(s_))
            if trace is not None:
                now = time.perf_counter()
                trace.append(("finish", s_, round((now - t_f) * 1e3, 3), "since prev finish", round((now - t_prev) * 1e3, 3)))
                t_prev = now
            last = (res if isinstance(res, list) else [res], which[s_])
            done += size[s_]
    if trace is not None:
        print("run_steps trace:", trace, file=sys.stderr, flush=True)
    return last


def exponent_sum(scalars_arr, exps_arr, order):
    """sum_i s_i e_i mod l for (n, 32) little-endian byte arrays: the exponent of B a commitment must equal"""
    return sum(int.from_bytes(bytes(x), "little") * int.from_bytes(bytes(y), "little")
               for x, y in zip(scalars_arr, exps_arr)) % order


def self_launch(args, argv):
    """`python3 bench.py --gpus N` started as ONE plain process (no WORLD_SIZE): be the launcher.  N child processes,
    one rank per GPU (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment - what torch.distributed.run
    would set), started BEFORE anything in this process touches the GPU; never exec.  Rank 0's JSON line is relayed
    as the LAST line of stdout, everything else the children print goes to stderr, and the exit status is the worst
    child's.  If the native (RCCL) exchange fails on the first attempt the run is repeated ONCE with the partial
    points carried by torch.distributed (--comm torch), so a launch detail cannot cost the whole measurement."""
    import signal
    import socket
    import subprocess
    import threading

    def free_port():
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
            sk.bind(("127.0.0.1", 0))
            return sk.getsockname()[1]

    live = []

    def forward(signum, _frame):
        # the launcher is being stopped: take the ranks (own process groups) along, then go
        for pr in list(live):
            if pr.poll() is None:
                try:
                    os.killpg(pr.pid, signal.SIGKILL)
                except Exception:
                    pr.kill()
        os._exit(128 + signum)
    for sg in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):
        try:
            signal.signal(sg, forward)
        except Exception:
            pass

    def attempt(extra):
        env0 = dict(os.environ)
        env0.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL needs it on this driver
        env0.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(free_port()), "WORLD_SIZE": str(args.gpus),
                     "LOCAL_WORLD_SIZE": str(args.gpus), "VMPC_BENCH_SELF_LAUNCHED": "1"})
        procs, last = [], {"line": None}
        for r in range(args.gpus):
            env = dict(env0, RANK=str(r), LOCAL_RANK=str(r))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv + extra, env=env,
                                          stdout=subprocess.PIPE, stderr=None, text=True, start_new_session=True))
            live.append(procs[-1])

        def pump(r, pr):
            for ln in pr.stdout:
                ln = ln.rstrip("\n")
                if r == 0 and ln.startswith('{"metric"'):
                    last["line"] = ln
                else:
                    print(f"[rank {r}] {ln}", file=sys.stderr, flush=True)
        pumps = [threading.Thread(target=pump, args=(r, pr), daemon=True) for r, pr in enumerate(procs)]
        for t_ in pumps:
            t_.start()
        # one rank gone with an error: the others cannot finish a collective - give them a grace period, then end
        # exactly the processes started here (by pid / process group, never by pattern)
        deadline = None
        while any(pr.poll() is None for pr in procs):
            time.sleep(0.2)
            codes = [pr.poll() for pr in procs]
            if deadline is None and any(c not in (None, 0) for c in codes):
                deadline = time.time() + 30.0
            if deadline is not None and time.time() > deadline:
                for pr in procs:
                    if pr.poll() is None:
                        try:
                            os.killpg(pr.pid, signal.SIGKILL)
                        except Exception:
                            pr.kill()
        for t_ in pumps:
            t_.join(timeout=5.0)
        codes = [pr.wait() for pr in procs]
        worst = max((abs(c) for c in codes), default=0)
        return worst, last["line"], codes

    worst, line, codes = attempt([])
    failed = worst != 0 or line is None or "error" in json.loads(line)
    if failed and args.comm == "native" and args.dist_backend == "nccl" and "--comm" not in argv:
        print(f"bench.py launcher: first attempt failed (exit codes {codes}); repeating with --comm torch",
              file=sys.stderr, flush=True)
        worst2, line2, codes2 = attempt(["--comm", "torch"])
        if line2 is not None and worst2 == 0:
            d = json.loads(line2)
            d.setdefault("config", {})["launcher_note"] = \
                f"native exchange failed on the first attempt (exit codes {codes}); this line is the --comm torch rerun"
            worst, line = worst2, json.dumps(d)
    if line is None:
        line = json.dumps({"metric": "Ed25519 MSM scalar-mults/sec", "value": None, "unit": "scalar-mults/s",
                           "n_gpus": args.gpus, "error": f"no rank-0 line; child exit codes {codes}"})
        worst = worst or 1
    sys.stderr.flush()
    print(line, flush=True)
    return worst


def dump_outputs(out_dir, results, result_idx):
    """--dump-outputs DIR: what the timed path hands its caller in the last step - the commitments of the last launch,
    each as its canonical affine bytes (x then y, 32 bytes each, little-endian; every byte exact in float32) - and
    which of the seeded scalar vectors each one commits to."""
    os.makedirs(out_dir, exist_ok=True)
    aff = np.array([np.frombuffer(pt.to_affine_bytes(), np.uint8) for pt in results], dtype=np.float32)
    np.save(os.path.join(out_dir, "commitments_affine_bytes.npy"), aff)
    np.save(os.path.join(out_dir, "commitments_scalar_vector_index.npy"), np.asarray(result_idx, dtype=np.float32))


def oracle_commitment_check(points_affine, scalar_arrs, need, got):
    """Every commitment in `got` ({scalar-vector index: point}) recomputed by the oracle's C restatement of the
    reference algorithm over the same host arrays; asserts equality of the canonical affine bytes."""
    from oracle import c_oracle
    t0 = time.perf_counter()
    threads = c_oracle.host_threads()
    prev = c_oracle.set_threads(threads)
    try:
        zero = np.zeros(32, np.uint8)
        ident = np.zeros(64, np.uint8)
        ident[32] = 1                                        # (0, 1): h ** 0 times the product
        for i in need:
            _, want = c_oracle.vector_commitment(scalar_arrs[i], zero, points_affine, ident)
            assert got[i].to_affine_bytes() == bytes(want), f"commitment {i} differs from the C oracle"
    finally:
        c_oracle.set_threads(prev)
    return {"commitments": len(need), "threads": threads, "seconds": round(time.perf_counter() - t0, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)       # 60 ms timed region per generator form
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline (see the module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the commitments of the last timed step to DIR/*.npy (float32)")
    ap.add_argument("--repeats", type=int, default=None,
                    help="back-to-back repetitions of the K-step timed region; the line reports their median "
                         "(default: 1, with --full 5)")
    ap.add_argument("--log2n", type=int, default=20, help="MSM terms per GPU = 2^log2n")
    ap.add_argument("--cpu-log2n", type=int, default=17, help="cpu_baseline sample size")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prove", action="store_true")
    ap.add_argument("--force-collective", action="store_true",
                    help="run the all-gather + ordered combine even with one rank (self-test)")
    ap.add_argument("--dist-backend", choices=("nccl", "gloo"), default=os.environ.get("VMPC_DIST_BACKEND", "nccl"),
                    help="torch.distributed backend of the process group.  gloo: the partial points are staged "
                         "through host memory (tests: several ranks may share one GPU)")
    ap.add_argument("--comm", choices=("native", "torch"), default=os.environ.get("VMPC_COMM", "native"),
                    help="native: the exchange runs inside libvmpc_hip (ncclAllGather on the MSM's stream, "
                         "include/vmpc.h vmpc_comm_*), bootstrapped over torch.distributed; torch: "
                         "torch.distributed carries the partial points (fallback when the native communicator "
                         "cannot be created)")
    ap.add_argument("--sharded-prove", action="store_true",
                    help="time the sharded compact prover also with one rank (--force-collective); with more "
                         "than one rank it is timed by default (--no-sharded-prove to skip)")
    ap.add_argument("--no-sharded-prove", action="store_true")
    ap.add_argument("--sharded-log2n", type=int, default=20,
                    help="N of the sharded prove section; with more than one rank it is also timed at N * world "
                         "(2^20 generators per rank: weak scaling - at N = 2^20 over 8 ranks the rounds are latency-bound)")
    ap.add_argument("--config4-log2n", type=int, default=24,
                    help="with more than one rank: total terms (log2) of the BASELINE config-4 commitment, sharded "
                         "cyclically over the ranks (2^24 over 8 GPUs = 2^21 per rank); 0 = skip")
    ap.add_argument("--variable-base", action="store_true",
                    help="headline on generators given as plain affine points (prepared per call) instead of "
                         "generators resident in prepared form; the other mode is always reported beside it")
    ap.add_argument("--batch", type=int, default=int(os.environ.get("VMPC_BENCH_BATCH", "3")),
                    help="commitments per launch over the prepared generators (vmpc_msm_table_batch_dev): the "
                         "reduction and recombination chains are paid once per batch; 1 = one commitment per launch")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="one commitment in flight (default: 3 launches, on three streams of the same GPU)")
    ap.add_argument("--table-rows", type=int, default=int(os.environ.get("VMPC_BENCH_TABLE_ROWS", "13")),
                    help="rows of the resident generator table: 13 = the wide-window table (rows spaced 20 bits, 13 mixed "
                         "additions per term, what pivot._auto_tabulate builds for a CRS of >= 2^19 generators; default "
                         "since round 6), 1 = prepared form only (no multiples; the headline of rounds 2-5, still timed "
                         "and reported beside it), 2/4/8/16 = 16-bit-window table with rows - 1 extra multiples")
    ap.add_argument("--depth", type=int, default=int(os.environ.get("VMPC_BENCH_DEPTH", "0")),
                    help="launches in flight (streams of the same GPU); 0 = the measured optimum")
    ap.add_argument("--watchdog-s", type=float, default=float(os.environ.get("VMPC_BENCH_WATCHDOG_S", "1500")),
                    help="give up (JSON line with an error entry, exit status 3) after this long")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started plain (as the N = 1 line is): start the N ranks ourselves, as children, before any GPU call
        sys.exit(self_launch(args, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    gpu_clocks = clocks_sample() if rank == 0 and args.full else None    # before anything below initialises the GPU
    sampler = ClockSampler() if rank == 0 and args.full else None        # (likewise: its child starts before GPU init)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    import torch
    ndev = torch.cuda.device_count()
    assert ndev >= 1, "no GPU visible: the AC20 hot path has no CPU fallback"
    # one process per GPU; only the host-staged gloo mode lets ranks share a device (2-rank tests on a 1-GPU box)
    assert args.dist_backend == "gloo" or local_rank < ndev, f"LOCAL_RANK {local_rank} but {ndev} GPU(s) visible"
    device_index = local_rank % ndev
    torch.cuda.set_device(device_index)
    dist = None
    state = {"line": None, "stage": "init"}
    import threading
    if os.environ.get("VMPC_BENCH_STACKS_AFTER_S"):          # debugging aid: Python stacks of a run that stalls
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["VMPC_BENCH_STACKS_AFTER_S"]), repeat=True)

    # A stuck kernel or collective must not look like success, nor hang the harness: report what there is and leave
    # with a failure status.  Stages that contain a first collective have a budget of their own, so that a launch that
    # cannot communicate is over in minutes (the self-launcher then repeats the run with --comm torch).
    stage_budget = {"init": 300.0, "communicator": 300.0, "warm-up": 420.0}
    t_start = time.time()

    def enter(stage):
        state["stage"], state["since"] = stage, time.time()
        if world > 1:            # a multi-rank run that stalls should say where, in the launcher's log
            print(f"[bench rank {rank}] +{time.time() - t_start:6.1f} s  {stage}", file=sys.stderr, flush=True)
    state["since"] = t_start

    def give_up(why):
        line = state["line"] or {"metric": "Ed25519 MSM scalar-mults/sec", "value": None, "unit": "scalar-mults/s",
                                 "n_gpus": world}
        line["error"] = f"rank {rank}: {why} (stage: {state['stage']})"
        print(json.dumps(line), flush=True)
        os._exit(3)

    def watch():
        while True:
            time.sleep(1.0)
            now = time.time()
            if now - t_start > args.watchdog_s:
                give_up(f"no result within {args.watchdog_s:.0f} s")
            budget = stage_budget.get(state["stage"])
            if budget is not None and now - state["since"] > budget:
                give_up(f"stage made no progress within {budget:.0f} s")
    watchdog = threading.Thread(target=watch, daemon=True)
    watchdog.start()
    if world > 1 or args.force_collective:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    def barrier():
        if dist:
            dist.barrier()

    import verifiable_mpc_amd as vm
    from verifiable_mpc_amd import parallel
    ctx = vm.get_context()
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)

    # ---- the exchange: inside the C library when possible -------------------------------------------------
    # one communicator PER commitment slot (each slot = a stream of its own): parallel.make_comms
    comm, comms, comm_kind, comm_note, comm_info = None, [], "none", None, None
    n_slots_env = int(os.environ.get("VMPC_MSM_SLOTS", "3"))
    if dist:
        enter("communicator")
        want = "host" if args.dist_backend == "gloo" else ("rccl" if args.comm == "native" else None)
        if want:
            try:
                comms = parallel.make_comms(ctx, world, rank, dist, torch, transport=want,
                                            count=1 if args.no_pipeline else n_slots_env)
            except Exception as e:
                comms, comm_note = [], f"{type(e).__name__}: {e}"
            # all or nothing: one rank without the native communicators puts every rank on torch.distributed
            flags = [None] * world
            dist.all_gather_object(flags, bool(comms))
            if not all(flags):
                for c_ in comms:
                    c_.close()
                comms = []
                assert args.dist_backend == "nccl", f"host-staged communicator failed: {comm_note}"
        comm = comms[0] if comms else None
        comm_kind = comm.kind if comm is not None else "torch.distributed"
        # what the LIBRARY says about its communicators (an RCCL one asks ncclCommCount / ncclCommUserRank): the
        # answer to "did the exchange really span N ranks" does not rest on WORLD_SIZE
        if comms:
            infos = [c_.info() for c_ in comms]
            assert all(i["world"] == world and i["rank"] == rank for i in infos), f"communicator disagrees: {infos}"
            comm_info = {"kind": infos[0]["kind"], "world": infos[0]["world"], "communicators": len(infos),
                         "source": "vmpc_comm_info"}
        else:
            comm_info = {"kind": "torch.distributed", "world": dist.get_world_size(), "communicators": 0,
                         "source": "torch.distributed.get_world_size"}

    n = 1 << args.log2n
    rng = np.random.default_rng(20200152 + 1 + rank)
    group = vm.EllipticCurve("Ed25519", "projective")
    # synthetic inputs (SURVEY.md 8d cfg 2/4): g_i = r_i * B on the device, uniform scalars
    exps_arr = rand_scalars(rng, n)
    exps = vm.ScalarVector.from_array(exps_arr)
    points = vm.PointVector.fixed_base(group.generator, exps, keep_proj=False)
    batch = 1 if (args.no_pipeline or args.variable_base) else max(1, min(args.batch, 16))
    # the commitments of one launch are over DISTINCT scalar vectors (A_i / B_i of a round, or queued independent
    # commitments - never the same vector twice)
    scalar_arrs = [rand_scalars(rng, n) for _ in range(max(batch, 1))]
    scalar_vectors = [vm.ScalarVector.from_array(a) for a in scalar_arrs]
    # The generators of a Pedersen commitment are a CRS (circuit_sat_r1cs.py:47-93 creates them once, every
    # commitment reuses them), so by default they are RESIDENT IN PREPARED FORM: the (y-x, y+x, 2dxy) image of
    # each affine point, one 128-byte line, computed once at CRS load (untimed) - a representation of the same
    # 2^20 points, no multiples of them.  `variable_base` = the same commitment from plain affine points,
    # converted inside every call (k_msm_prep); both modes are timed and reported.
    points_prepared = vm.PointVector(points.a, None, ctx).precompute([], rows=args.table_rows)
    points_plain = points
    if not args.variable_base:
        points = points_prepared
    shard = parallel.ShardedMsm(ctx, world, rank, dist, torch, force_collective=args.force_collective,
                                comm=comms if comms else None)
    depth = 1 if args.no_pipeline else (min(args.depth, shard.n_slots) if args.depth > 0 else shard.n_slots)

    def steps(k, pts):
        return run_steps(shard, k, scalar_vectors, pts, depth, batch)

    def grow_workspaces(pts):
        """one full-size launch on every slot, untimed: each slot's context sizes its scratch arena on first use
        (a hipMalloc), which must not land in the timed region when the W warm-up steps do not reach every slot"""
        per = batch if getattr(pts, "_table", None) is not None else 1
        for slot in range(depth):
            shard.finish(shard.launch(scalar_vectors[:per] if per > 1 else scalar_vectors[0], pts, slot))

    # A full (generation-2) pass of Python's cyclic collector over a process that has imported torch takes
    # 40-50 ms, and WHEN it runs depends on how many container objects the loop below has allocated: it landed in
    # the timed region for some --batch / --steps combinations and not for others (2.9 instead of 1.1 ms per
    # step).  Collect now and move everything that exists to the permanent generation; collections during the
    # timed regions then only look at the few objects made since.
    import gc
    gc.collect()
    gc.freeze()
    enter("warm-up")
    grow_workspaces(points)
    if args.warmup:
        steps(args.warmup, points)
    torch.cuda.synchronize()
    barrier()
    prof_ctxs = list(getattr(shard.backend, "ctxs", [ctx]))[:depth]

    def timed(pts, reps):
        """`reps` repetitions of EXACTLY K steps, each bracketed by barrier + device synchronisation on both sides,
        max over ranks; no stage events on the streams.  Returns (seconds per repetition, result of the last)."""
        runs, res = [], None
        for _ in range(reps):
            torch.cuda.synchronize()
            barrier()
            t0 = time.perf_counter()
            res = steps(args.steps, pts)
            torch.cuda.synchronize()
            barrier()
            dt = time.perf_counter() - t0
            if dist:
                t = torch.tensor([dt], dtype=torch.float64, device="cuda" if args.dist_backend == "nccl" else "cpu")
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt = float(t.item())
            runs.append(dt)
        return runs, res

    enter("timed region")
    # the headline: median of `--repeats` back-to-back repetitions of the K-step region (--full: five; one 20-60 ms
    # window used to decide it; boxes and windows differ by several per cent), min / max reported beside it
    t_region0 = time.time()
    elapsed_runs, (results, result_idx) = timed(points, args.repeats)
    t_region1 = time.time()
    elapsed = sorted(elapsed_runs)[len(elapsed_runs) // 2]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, results, result_idx)
    checked, oracle_check = False, None
    if args.full:
        # once more with the per-stage HIP events on every stream the kernels are launched on: the in-region kernel
        # durations of the roofline entry (not part of the headline: the events themselves cost time)
        timed_profile = os.environ.get("VMPC_BENCH_TIMED_PROFILE", "1") != "0"
        prof = {}
        if timed_profile:
            for c_ in prof_ctxs:
                c_.profile(True)
                c_.profile_read(reset=True)
            torch.cuda.synchronize()
            barrier()
            steps(args.steps, points)
            torch.cuda.synchronize()
            barrier()
            for c_ in prof_ctxs:       # HIP events on each stream the kernels were launched on
                for name, (ms, cnt) in c_.profile_read(reset=True).items():
                    a, b = prof.get(name, (0.0, 0))
                    prof[name] = (a + ms, b + cnt)
                c_.profile(False)
        ctx.sync()

        # outside the timed region: the same commitment alone on the GPU (one in flight), so that
        # the per-stage durations are not stretched by the other in-flight commitments' kernels,
        # and the integer-ALU ceiling the bucket stage is priced against
        enter("one commitment alone")
        iso, alu_peak, iso_ms, iso_steps = {}, None, None, 5
        c0 = prof_ctxs[0]
        # (every rank: with a collective the launches are collective too)
        for _ in range(2):
            shard.finish(shard.launch(scalar_vectors[0], points, 0))
        t1 = time.perf_counter()
        for _ in range(iso_steps):             # latency: no stage events on the stream (they cost ~0.1 ms per commitment)
            shard.finish(shard.launch(scalar_vectors[0], points, 0))
        iso_ms = (time.perf_counter() - t1) / iso_steps * 1e3
        if rank == 0:
            c0.profile(True)
            c0.profile_read(reset=True)
        for _ in range(iso_steps):             # the same again with the per-stage HIP events: the roofline's kernel time
            shard.finish(shard.launch(scalar_vectors[0], points, 0))
        busy_clocks = None
        if rank == 0:
            iso = {k: ms / max(c, 1) for k, (ms, c) in c0.profile_read(reset=True).items()}
            c0.profile(False)
            alu_peak = max(c0.madd_rate(400) for _ in range(3))
        if rank == 0 and sampler is not None and not shard.collective:
            # the clocks the alone-kernel figures were taken at: the same commitment back to back for ~0.25 s while the
            # child samples sclk / power (the 5-launch loops above are over before two samples are in)
            t_a0 = time.time()
            while time.time() - t_a0 < 0.25:
                shard.finish(shard.launch(scalar_vectors[0], points, 0))
            t_a1 = time.time()
            time.sleep(0.02)
            try:        # the card this process computes on, by PCI address (the box's sysfs shows every GPU of the node)
                pr = torch.cuda.get_device_properties(device_index)
                pci = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
            except Exception:
                pci = None
            busy_clocks = {"one_commitment_alone_loop": sampler.window(t_a0, t_a1, pci),
                           "timed_region": sampler.window(t_region0, t_region1, pci),
                           "source": "sysfs pp_dpm_sclk / pp_dpm_mclk / hwmon power1_average, read every ~5 ms by a child "
                                     "process started before GPU initialisation"}
        if sampler is not None:
            sampler.stop()
        # (for comparison) one commitment alone over a 4-row fixed-base table of the same generators (what a CRS
        # that serves many commitments holds; 3 extra multiples per generator): the recombination chain is 48 doublings
        # instead of 240 and the reduction covers 4 bucket sets instead of 16
        alone_table = None
        if rank == 0 and not args.variable_base and os.environ.get("VMPC_BENCH_ALONE_TABLE", "1") != "0":
            try:
                tab = vm.PointVector(points_plain.a, None, ctx).precompute([], rows=4)
                t_, res_ = tab._table, ctx.alloc(128)
                for _ in range(2):
                    ctx.msm_table(t_.ptr, t_.n, 0, scalar_vectors[0].ptr, n, None, res_.ptr, None, rows=4)
                ctx.sync()
                t3 = time.perf_counter()
                for _ in range(iso_steps):
                    ctx.msm_table(t_.ptr, t_.n, 0, scalar_vectors[0].ptr, n, None, res_.ptr, None, rows=4)
                    ctx.sync()
                alone_table = {"rows": 4, "table_MiB": (4 * n * 128) >> 20,
                               "ms_per_commitment": round((time.perf_counter() - t3) / iso_steps * 1e3, 4)}
                got = vm.Ed25519Point.from_proj_bytes(ctx.download(res_.ptr, 128).tobytes()[:96]).normalize()
                alone_table["same_point_as_prepared_form"] = bool(got == shard.finish(shard.launch(scalar_vectors[0], points, 0))) \
                    if not shard.collective else None
                del tab, t_, res_
            except Exception as e:
                alone_table = {"error": f"{type(e).__name__}: {e}"}
        # the other generator form, same K steps, same brackets
        enter("other generator form")
        other_pts = points_plain if points is points_prepared else points_prepared
        grow_workspaces(other_pts)
        if args.warmup:
            steps(args.warmup, other_pts)
        other_runs, (other_results, other_idx) = timed(other_pts, args.repeats)
        other_elapsed = sorted(other_runs)[len(other_runs) // 2]
        # ... and, when the headline runs over a table of multiples, the prepared form WITHOUT multiples (one 128-byte line
        # per generator: the headline of rounds 2-5)
        prepared1 = None
        if not args.variable_base and args.table_rows != 1:
            enter("prepared form without multiples")
            p1 = vm.PointVector(points_plain.a, None, ctx).precompute([], rows=1)
            grow_workspaces(p1)
            if args.warmup:
                steps(args.warmup, p1)
            p1_runs, (p1_results, p1_idx) = timed(p1, max(1, args.repeats - 2))
            p1_elapsed = sorted(p1_runs)[len(p1_runs) // 2]
            prepared1 = {"value": world * n * args.steps / p1_elapsed, "ms_per_step": p1_elapsed / args.steps * 1e3,
                         "table_MiB": (n * 128) >> 20,
                         "note": "same K steps and brackets; generators as one prepared 128-byte line each, 16 mixed "
                                 "additions per term (16-bit windows) + recombination"}
            if not shard.collective:
                same = {i: pt for pt, i in zip(results, result_idx)}
                prepared1["same_points_as_headline"] = all(pt == same[i] for pt, i in zip(p1_results, p1_idx) if i in same)
            del p1
        no_check = bool(os.environ.get("BENCH_NO_CHECK"))          # (developer A/B builds that break the result)

        # size-independent correctness property at full size, for every commitment of the last launch:
        #     sum_i s_i * (e_i * B) == (sum_i s_i e_i mod l) * B,     the sum running over ALL ranks' shards
        enter("result check")
        if not no_check:
            need = sorted(set(result_idx) | set(other_idx))
            mine = {i: exponent_sum(scalar_arrs[i], exps_arr, vm.groups.ORDER) for i in need}
            if dist:
                every = [None] * world
                dist.all_gather_object(every, mine)
                assert all(sorted(e) == need for e in every), "ranks disagree on which commitments ran last"
                tot = {i: sum(e[i] for e in every) % vm.groups.ORDER for i in need}
            else:
                tot = mine
            want = vm.PointVector.fixed_base(group.generator, [tot[i] for i in need], keep_proj=False)
            want = {i: want[j] for j, i in enumerate(need)}
            for res, idx in ((results, result_idx), (other_results, other_idx)):
                for pt, i in zip(res, idx):
                    assert pt == want[i], f"MSM property check failed (rank {rank}, scalar vector {i})"
            checked = True
            if world == 1 and os.environ.get("VMPC_BENCH_ORACLE_CHECK", "1") != "0":
                # and bit for bit against the C restatement of the REFERENCE algorithm (pivot.py:139-145: a ladder per
                # term + the product tree; oracle/ed25519_oracle.c, ladders spread over the host's cores) - the same
                # library the cpu_baseline leg times, here as the checker only, outside every timed region
                oracle_check = oracle_commitment_check(points_plain.affine_array(), scalar_arrs, need,
                                                       {i: pt for res, idx in ((results, result_idx),
                                                                               (other_results, other_idx))
                                                        for pt, i in zip(res, idx)})

    line = None
    if rank == 0:
        value = world * n * args.steps / elapsed
        line = {
            "metric": "Ed25519 MSM scalar-mults/sec", "value": value,
            "unit": "scalar-mults/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u32 (255-bit modular integers as 10 limbs of 25.5 bits, 32x32->64 multiply-adds)", "data": "synthetic",
            "checked": checked,
            "checked_how": (f"C oracle (reference algorithm: one double-and-add ladder per term + product tree, "
                            f"pivot.py:139-145), bit-exact on the affine result of {oracle_check['commitments']} "
                            f"commitment(s) of n=2^{args.log2n} from the last timed launches, "
                            f"{oracle_check['threads']} host threads, {oracle_check['seconds']} s, outside the timed "
                            f"region; and the exponent identity on all of them"
                            if oracle_check else
                            "exponent identity sum_i s_i (e_i B) == (sum_i s_i e_i mod l) B across ranks against the "
                            "product's fixed-base kernel (N > 1: each rank holds a shard; the single-GPU line and "
                            "tests/test_gpu_full_size.py check against the C oracle bit for bit)"
                            if checked else
                            "not checked in a plain run: bench.py --full checks the commitments of the last timed "
                            "launches (exponent identity; on one GPU also bit for bit against the C oracle)"),
            "config": {"workload": f"Pedersen vector-commitment MSM, n=2^{args.log2n} Ed25519 "
                                   f"generators per GPU, uniform 252-bit scalars",
                       "terms_per_gpu": n, "total_terms": world * n, "launches_in_flight": depth,
                       "commitments_per_launch": batch,
                       "scalar_vectors": f"{len(scalar_vectors)} distinct (one per commitment of a launch)",
                       "timing": {"throughput_ms_per_commitment": round(elapsed / args.steps * 1e3, 4),
                                  "repeats": len(elapsed_runs),
                                  "ms_per_step_of_each_repeat": [round(e / args.steps * 1e3, 4) for e in elapsed_runs],
                                  "ms_per_step_min": round(min(elapsed_runs) / args.steps * 1e3, 4),
                                  "ms_per_step_max": round(max(elapsed_runs) / args.steps * 1e3, 4),
                                  "headline": "median of the repeats (each: EXACTLY K steps between barrier + device "
                                              "synchronisation, max over ranks)"},
                       "generators": ("plain affine points, prepared inside every call" if args.variable_base else
                                      "resident in prepared form (128-byte niels image of each point, made once "
                                      "at CRS load, untimed)" if args.table_rows == 1 else
                                      f"resident as the 13-row WIDE-WINDOW fixed-base table (rows spaced 20 bits: 12 extra "
                                      f"multiples per generator, {(13 * n * 128) >> 20} MiB, made once at CRS load, untimed; "
                                      f"what pivot._auto_tabulate builds for a CRS committed to more than once)"
                                      if args.table_rows == 13 else
                                      f"resident as a {args.table_rows}-row fixed-base table ({args.table_rows - 1} extra "
                                      f"multiples per generator, made once at CRS load, untimed)"),
                       "collective": (f"all_gather(128 B/rank and commitment) + rank-ordered add, transport: {comm_kind}"
                                      if shard.collective else "none"),
                       "dist_backend": args.dist_backend if dist else None,
                       "comm": comm_info,
                       "launched_by": ("bench.py itself (child processes)" if os.environ.get("VMPC_BENCH_SELF_LAUNCHED")
                                       else "external launcher" if "WORLD_SIZE" in os.environ else "plain process"),
                       "run": "full (--full)" if args.full else "plain: headline only (--full measures the rest)"},
        }
        if comm_note:
            line["config"]["native_comm_error"] = comm_note
        state["line"] = line
    if rank == 0 and args.full:
        traffic = pmc_traffic_calibrated("k_msm_bucket")
        bucket_ms, bucket_n = prof.get("msm_bucket", (0.0, 0))
        t_bucket_timed = bucket_ms / max(bucket_n, 1) / 1e3          # in the timed region: three launches in flight
        c_bits, windows = ctx.msm_plan(n)
        if args.table_rows == 13 and not args.variable_base:
            c_bits, windows = 20, 13            # the wide-window table: thirteen 20-bit digits per scalar
        madds = n * windows                     # one mixed addition per non-zero digit (upper bound)
        iso_bucket_s = iso.get("msm_bucket", 0.0) / 1e3
        # The roofline figure uses the kernel ALONE on the GPU (one commitment in flight, same inputs, same
        # process): that is the duration rocprofv3 reports for it (profiles/*_alone_kernel_stats.csv agrees
        # within a few %).  With three launches in flight a HIP-event bracket also counts the time the
        # kernel's workgroups wait behind other streams' kernels; that figure is reported beside it.
        t_bucket = iso_bucket_s if iso_bucket_s > 0 else t_bucket_timed
        achieved = BYTES_PER_TERM * n / t_bucket / 1e9 if t_bucket > 0 else 0.0
        other_value = world * n * args.steps / other_elapsed
        var_value = value if args.variable_base else other_value
        line["config"]["timing"].update({
            # the DEFAULT path of a generator vector that is committed to more than once
            # (pivot._auto_tabulate: the 13-row wide-window table at 2^20); other forms beside it
            "latency_ms_one_commitment_alone":
                round(iso_ms, 4) if args.table_rows == 13 else
                (alone_table or {}).get("ms_per_commitment") or round(iso_ms, 4),
            "latency_ms_one_commitment_alone_form":
                ("13-row wide-window table (what a PointVector of >= 2^19 generators becomes at its "
                 "second commitment)" if args.table_rows == 13 else
                 f"{alone_table['rows']}-row fixed-base table" if (alone_table or {}).get("ms_per_commitment")
                 else "prepared generators"),
            "latency_ms_one_commitment_alone_4_row_table": (alone_table or {}).get("ms_per_commitment"),
            "latency_ms_one_commitment_alone_headline_form": round(iso_ms, 4),
            "what": "value = pipelined throughput (launches_in_flight x commitments_per_launch "
                    "commitments in flight); a prover's commitments are sequential and cost "
                    "the latency figure"})
        line["config"]["variable_base_scalar_mults_per_s"] = round(var_value, 1)
        line["config"]["gpu_clocks"] = {"idle_before_gpu_init": gpu_clocks, "busy": busy_clocks}
        line.update({
            "roofline": {"bound": "hbm", "kernel": "k_msm_bucket", "achieved": achieved,
                         "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                         "traffic": traffic["bytes"], "traffic_source": traffic["source"],
                         "traffic_detail": traffic["detail"],
                         "avg_kernel_ms": t_bucket * 1e3, "launches_timed": iso_steps,
                         "timing": "HIP events on the kernel's stream, the commitment alone on the GPU "
                                   "(5 launches after the timed region)",
                         "avg_kernel_ms_in_timed_region": t_bucket_timed * 1e3,
                         "launches_in_timed_region": bucket_n,
                         "commitments_per_launch_in_timed_region": batch,
                         "achieved_in_timed_region": (BYTES_PER_TERM * n * batch / t_bucket_timed / 1e9
                                                      if t_bucket_timed > 0 else None),
                         "algorithmic_bytes_per_launch": BYTES_PER_TERM * n,
                         "note": "255-bit modular-integer kernel: bound by 32x32 integer "
                                 "multiply-add issue, not HBM (DESIGN.md section 5); see `alu`",
                         "alu": {"unit": "G mixed-additions/s",
                                 "peak": alu_peak / 1e9,
                                 "peak_source": "vmpc_ed25519_madd_rate: register-resident 7M mixed "
                                                "additions on every lane, measured in this run",
                                 "achieved": madds / iso_bucket_s / 1e9 if iso_bucket_s else None,
                                 "frac": madds / iso_bucket_s / alu_peak if iso_bucket_s else None,
                                 "kernel_ms_alone": iso_bucket_s * 1e3,
                                 "mixed_additions_per_launch": madds,
                                 "window_bits": c_bits, "windows": windows}},
            ("prepared_generators" if args.variable_base else "variable_base"): {
                "value": other_value, "ms_per_step": other_elapsed / args.steps * 1e3,
                "note": "same K steps and brackets with the generators in the other form"},
            "prepared_generators_no_multiples": prepared1,
            "stages_us": {k: round(ms / max(c, 1) * 1e3, 1) for k, (ms, c) in prof.items()},
            "alone": {"over_fixed_base_table": alone_table,
                      "over_headline_form": {"ms_per_commitment": round(iso_ms, 4),
                                             "stages_us": {k: round(v * 1e3, 1) for k, v in iso.items()}}},
        })
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(args.cpu_log2n, 5)
            try:
                line["cpu_baseline"]["strong_cpu"] = strong_cpu_baseline(args.log2n, 8)
            except Exception as e:
                line["cpu_baseline"]["strong_cpu"] = {"error": f"{type(e).__name__}: {e}"}
            try:
                line["cpu_baseline"]["python_reference"] = python_reference_baseline(6)
            except Exception as e:
                line["cpu_baseline"]["python_reference"] = {"error": f"{type(e).__name__}: {e}"}
        if world == 1 and not args.no_prove and not args.force_collective:
            try:
                line["ac20_n2^20"] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in
                                      prove_timing(vm, ctx, 20, np.random.default_rng(99)).items()}
            except Exception as e:  # the headline metric must still be reported
                line["ac20_n2^20"] = {"error": f"{type(e).__name__}: {e}"}
            try:
                line["msm_other_sizes"] = other_sizes_timing(vm, ctx, (16, 21, 24))
            except Exception as e:
                line["msm_other_sizes"] = {"error": f"{type(e).__name__}: {e}"}
            try:
                line["msm_distributions"] = distribution_timing(vm, ctx, (16, 20))
            except Exception as e:
                line["msm_distributions"] = {"error": f"{type(e).__name__}: {e}"}
            try:
                line["bn256_n2^18"] = {k: (round(v, 2) if isinstance(v, float) else v)
                                       for k, v in bn256_timing(vm, ctx, 18).items()}
            except Exception as e:
                line["bn256_n2^18"] = {"error": f"{type(e).__name__}: {e}"}
            try:
                line["bn256_n2^18"].update(pinocchio_timing(vm, ctx, 18))
            except Exception as e:
                line["bn256_n2^18"]["whole_proof_error"] = f"{type(e).__name__}: {e}"
    sharded_info, sharded_weak, cfg4 = None, None, None
    if args.full and dist and world > 1 and args.config4_log2n > 0:
        enter("config 4")
        try:
            cfg4 = config4_timing(vm, parallel, shard, args.config4_log2n, world, rank, dist, barrier, torch)
        except Exception as e:
            cfg4 = {"error": f"{type(e).__name__}: {e}"}
    if dist and (args.sharded_prove or (args.full and world > 1 and not args.no_sharded_prove)):
        # every rank takes part; a failure here must not cost the headline line (a stuck collective ends in the
        # watchdog: line + error entry, exit status 3)
        enter("sharded prove")

        def run_sharded(lg):
            try:
                return {k: (round(v, 2) if isinstance(v, float) else v) for k, v in
                        sharded_prove_timing(vm, ctx, lg, world, rank, dist, torch, comm).items()}
            except Exception as e:
                return {"error": f"{type(e).__name__}: {e}"}
        sharded_info = run_sharded(args.sharded_log2n)
        if world > 1 and (world & (world - 1)) == 0:
            # weak scaling: 2^sharded_log2n generators PER RANK (the size at which a block is folded locally and the
            # rounds are not latency-bound)
            enter("sharded prove, weak scaling")
            sharded_weak = run_sharded(args.sharded_log2n + world.bit_length() - 1)
    enter("done")
    if rank == 0:
        if sharded_info is not None:
            line[f"ac20_n2^{args.sharded_log2n}_sharded"] = sharded_info
        if sharded_weak is not None:
            line[f"ac20_n2^{args.sharded_log2n + world.bit_length() - 1}_sharded_weak_scaling"] = sharded_weak
        if cfg4 is not None:
            line[f"msm_config4_n2^{args.config4_log2n}_over_{world}_gpus"] = cfg4
        if args.full:
            # the numbers a reader of the last 2000 characters of this line should see (a harness that keeps a tail of stdout
            # keeps THIS; everything here is also further up, with its context) - last key of the line on purpose
            try:
                a20, hf = line.get("ac20_n2^20") or {}, (line.get("ac20_n2^20") or {}).get("hash_floor") or {}
                busy = ((line["config"].get("gpu_clocks") or {}).get("busy") or {}).get("timed_region") or {}
                sizes = line.get("msm_other_sizes") or {}
                line["summary"] = {
                    "G_scalar_mults_per_s": round(line["value"] / 1e9, 4), "ms_per_step": round(line["ms_per_step"], 4),
                    "generators": f"{args.table_rows}-row table" if not args.variable_base else "plain points",
                    "same_run_prepared_form_ms_per_step": round((line.get("prepared_generators_no_multiples") or {}).get("ms_per_step") or 0, 4) or None,
                    "same_run_variable_base_ms_per_step": round((line.get("variable_base") or {}).get("ms_per_step") or 0, 4) or None,
                    "one_commitment_alone_ms": line["config"]["timing"].get("latency_ms_one_commitment_alone"),
                    "k_msm_bucket_alone_ms": round(line["roofline"]["avg_kernel_ms"], 4),
                    "roofline_frac_hbm": round(line["roofline"]["frac"], 5),
                    "alu_frac": round(line["roofline"]["alu"]["frac"] or 0, 4),
                    "traffic_GB_per_launch": round((line["roofline"]["traffic"] or 0) / 1e9, 3) or None,
                    "checked_against": "C oracle (reference algorithm), bit-exact" if oracle_check else "exponent identity",
                    "prove_ms_compact": a20.get("prove_ms_compact"), "verify_ms_compact": a20.get("verify_ms_compact"),
                    "prove_ms_reference": a20.get("prove_ms_reference"), "verify_ms_reference": a20.get("verify_ms_reference"),
                    "sha256_floor_ms": hf.get("hash_floor_ms"), "prove_over_floor": hf.get("prove_over_floor"),
                    "verify_over_floor": hf.get("verify_over_floor"),
                    "prove_outside_hash_ms": hf.get("prove_ms_outside_sha256_update"),
                    "verify_outside_hash_ms": hf.get("verify_ms_outside_sha256_update"),
                    "n2^16_ms_over_crs_table": (sizes.get("n2^16") or {}).get("ms_over_crs_table"),
                    "n2^21_ms_over_crs_table": (sizes.get("n2^21") or {}).get("ms_over_crs_table"),
                    "pinocchio_2^18_whole_proof_ms": (line.get("bn256_n2^18") or {}).get("whole_proof_ms"),
                    "busy_sclk_mhz_median": (busy.get("sclk_mhz") or {}).get("median"),
                    "busy_socket_power_w_median": (busy.get("socket_power_w") or {}).get("median"),
                    "cpu_reference_algorithm_1_core_per_s": round((line.get("cpu_baseline") or {}).get("value") or 0, 1) or None}
            except Exception as e:
                line["summary"] = {"error": f"{type(e).__name__}: {e}"}
        try:        # RCCL's version banner sits in the C stdio buffer: push it out first, the JSON line is the last line
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(line), flush=True)
    if dist:
        dist.barrier()
        for c_ in comms:
            c_.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
