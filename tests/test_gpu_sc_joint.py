"""GPU: coupled AMP from a beta_0 (k_scstart, sa_sc_amp_start), the staged coupled
context, the SPARC <-> LDPC glue on it and sc_joint.CoupledJointDecoder against
the NumPy statement tests/sc_joint_ref.py on the cases of tests/sc_joint_cases.py.
Tolerances: tests/test_gpu_sc.py's (norm-relative beta, per-entry phi)."""
import ctypes as ct

import numpy as np
import pytest

from conftest import golden
from oracle import amp_oracle as orc
from oracle import glue_oracle as go
import sc_cases
import sc_joint_cases as jc
import sc_joint_ref as ref

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "fp64": 1e-11}  # tests/test_gpu_sc.py's
STOP64 = 3
PRECS = ("fp32", "fp64")
D = ct.POINTER(ct.c_double)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd as s
    return s


_OPS = {}


def transforms(sp, case, prec):
    key = (case.L, case.M, case.n, case.omega, case.Lambda, prec)
    if key not in _OPS:
        Ab, Az, ordering = sp.sc_transforms(case.L, case.M, case.n, case.W, precision=prec, device=0)
        assert np.array_equal(ordering, case.ordering)
        _OPS[key] = (Ab, Az)
    return _OPS[key]


_CODE = {}


def ldpc_code(sp):
    if "c" not in _CODE:
        _CODE["c"] = sp.code("802.16", "5/6", 8, device=0)
    return _CODE["c"]


_JD = {}


def decoder(sp, case):
    if case.name not in _JD:
        _JD[case.name] = sp.CoupledJointDecoder(case.L, case.M, case.n, case.W, ldpc_code(sp), jc.T, device=0)
    return _JD[case.name]


# ---- the three starts -------------------------------------------------------------------
_STARTS = {}


def starts(case):
    """y of RandomState(1)'s rep and the three starts: soft (glue_oracle.soft_beta0 of a random app over every
    section), the true codeword with every fifth section moved to a wrong column, and zeros."""
    if case.name not in _STARTS:
        idx, y = case.rep(1)
        L, M, n = case.L, case.M, case.n
        rs = np.random.RandomState(17)
        soft = np.asarray(go.soft_beta0(np.zeros((1, L * M)), rs.randn(1, L * case.lgm) * 3, n, case.Pl, L, M, 0, L),
                          dtype=np.float64)[0]
        moved = np.where(np.arange(L) % 5 == 0, (idx + 1) % M, idx)
        wrong = np.zeros(L * M)
        wrong[np.arange(L) * M + moved] = np.sqrt(n * case.Pl)
        out = {}
        for name, b0 in (("soft", soft), ("wrong", wrong), ("zeros", np.zeros(L * M))):
            _, _, phi, _, snaps, _ = ref.amp_sc_start(y, case.Pl, case.W, L, M, 8, case.A, beta0=b0, early_stop=False)
            b0.setflags(write=False)
            phi.setflags(write=False)
            out[name] = (b0, phi, snaps)
        _STARTS[case.name] = (y, out)
    return _STARTS[case.name]


# ---- a. the beta_0-start trajectory ---------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("start", ["soft", "wrong", "zeros"])
@pytest.mark.parametrize("case", jc.START_CASES, ids=lambda c: c.name)
def test_start_trajectory(sp, case, start, prec):
    Ab, Az = transforms(sp, case, prec)
    y, st = starts(case)
    b0, phi_ref, snaps = st[start]
    for T in (1, 2, 4, 8):
        beta, iters, phi = sp.amp_sc_batch(y.reshape(1, -1), case.Pl, T, Ab, early_stop=False, beta0=b0.reshape(1, -1))
        assert beta.shape == (1, case.L * case.M) and phi.shape == (1, T, case.R) and iters[0] == T
        e_b = rel(beta, snaps[T])
        e_p = np.abs(phi[0] / phi_ref[:T] - 1).max()
        print(f"case {case.name} start {start} {prec} T={T}: beta {e_b:.2e} phi {e_p:.2e}")
        assert e_b <= TOL[prec], (T, e_b)
        assert e_p <= TOL[prec], (T, e_p)
    # the single-codeword form, in amp()'s order, both shapes of the start
    one = sp.amp_sc(y, case.Pl, case.L, case.M, 8, Ab, Az, b0, early_stop=False)
    assert np.array_equal(one.reshape(-1), beta[0])
    assert np.array_equal(sp.amp_sc(y, case.Pl, case.L, case.M, 8, Ab, Az, b0.reshape(-1, 1), early_stop=False), one)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", jc.START_CASES, ids=lambda c: c.name)
def test_zero_start_is_todays_decode_bit_for_bit(sp, case, prec):
    Ab, Az = transforms(sp, case, prec)
    y, _ = starts(case)
    ys = np.stack([y, case.rep(2)[1]])
    for es in (False, True):
        want = sp.amp_sc_batch(ys, case.Pl, 12, Ab, early_stop=es)
        zeros = sp.amp_sc_batch(ys, case.Pl, 12, Ab, early_stop=es, beta0=np.zeros((2, case.L * case.M)))
        none = sp.amp_sc_batch(ys, case.Pl, 12, Ab, early_stop=es, beta0=None)
        for a, b, c in zip(want, zeros, none):
            assert np.array_equal(a, b) and np.array_equal(a, c)
    got = sp.amp_sc(ys[0], case.Pl, case.L, case.M, 12, Ab, Az, np.array([None]))  # the reference's sentinel
    assert np.array_equal(got.reshape(-1), sp.amp_sc_batch(ys[:1], case.Pl, 12, Ab)[0][0])


# ---- b. stop with a start ------------------------------------------------------------------
# The decoded reps, as tests/sc_cases.py means it: the statement decodes every section and every one of its AMP calls,
# the first (from zero) included, reaches the bit-equality stop with STOP64 to spare.  A rep whose zero-start decode never
# reaches bit equality in T iterations sits on a last-place limit cycle, and where such a decode stops depends on the
# summation order: K1 seed 6 (first call runs out at 30, restart stops at 16 in the statement) is held to 1.7e-16 in beta
# by the MI355X (test_forced_inputs) and does not reach bit equality there in 30 iterations.
DECODED = [(c, s) for c in jc.JOINT_CASES for s in c.exact("soft")
           if max(c.recorded(s, "soft")["stops"]) < jc.T - STOP64 and c.recorded(s, "soft")["amp"][-1] == 0]


@pytest.mark.parametrize("case,seed", DECODED, ids=lambda v: getattr(v, "name", str(v)))
def test_stop_after_a_soft_restart(sp, case, seed):
    Ab, Az = transforms(sp, case, "fp64")
    r = jc.rep(case, seed, "soft")
    b0 = np.asarray(go.soft_beta0(r["betas"][0][None, :], r["apps"][0][None, :], case.n, case.Pl, case.L, case.M,
                                  case.l0, case.ns), dtype=np.float64)
    beta, iters, phi = sp.amp_sc_batch(r["y"].reshape(1, -1), case.Pl, jc.T, Ab, beta0=b0)
    stop, want = int(iters[0]), r["stops"][1]
    print(f"case {case.name} seed {seed}: stop {stop} (statement {want})")
    assert abs(stop - want) <= STOP64
    assert np.array_equal(beta.reshape(case.L, case.M).argmax(axis=1), r["betas"][1].reshape(case.L, case.M).argmax(axis=1))
    assert np.all(phi[0, stop:] == 0) and np.all(phi[0, :stop] > 0)


# ---- c. batch independence, one-call == staged ----------------------------------------------
@pytest.mark.parametrize("early_stop", [False, True], ids=["nostop", "stop"])
@pytest.mark.parametrize("prec", PRECS)
def test_batch_with_starts_is_its_codewords_and_the_staged_calls(sp, prec, early_stop):
    case = jc.K2
    Ab, Az = transforms(sp, case, prec)
    op = Ab.op
    y, st = starts(case)
    ys = np.stack([y, case.rep(2)[1], case.rep(3)[1]])
    b0 = np.stack([st["soft"][0], st["wrong"][0], st["zeros"][0]])
    T = 12
    beta, iters, phi = sp.amp_sc_batch(ys, case.Pl, T, Ab, early_stop=early_stop, beta0=b0)
    for k in range(3):
        b1, i1, p1 = sp.amp_sc_batch(ys[k:k + 1], case.Pl, T, Ab, early_stop=early_stop, beta0=b0[k:k + 1])
        assert np.array_equal(b1[0], beta[k]) and i1[0] == iters[k] and np.array_equal(p1[0], phi[k])
    op.reserve(3, T)
    op.stage(ys, case.Pl, beta0=b0)
    for _ in range(2):  # the staged y survives a run; the start is staged again
        op.run(3, T, early_stop=early_stop, beta0=True)
        op.wait()
        assert np.array_equal(op.fetch_beta(3), beta) and np.array_equal(op.iters(3), iters)
        assert np.array_equal(op.fetch_phi(3, T), phi)
        assert np.array_equal(op.decide(3), beta.reshape(3, case.L, case.M).argmax(axis=2))
        op.stage(ys, beta0=b0)
    # without SA_FLAG_BETA0 the staged y decodes from zero, as the one-call entry point does
    op.run(3, T, early_stop=early_stop)
    op.wait()
    assert np.array_equal(op.fetch_beta(3), sp.amp_sc_batch(ys, case.Pl, T, Ab, early_stop=early_stop)[0])


# ---- d. tolerances with a start ----------------------------------------------------------------
@pytest.mark.parametrize("which", ["stop_tol", "freeze_tol"])
def test_tolerances_with_a_start(sp, which):
    case = jc.K1
    y, st = starts(case)
    b0 = st["soft"][0]
    kw = dict(stop_tol=0.01) if which == "stop_tol" else dict(freeze_tol=0.05)
    T = jc.T
    want = ref.amp_sc_start(y, case.Pl, case.W, case.L, case.M, T, case.A, beta0=b0, **kw)
    frozen = int((want[3][:want[1]] == 0).sum())
    print(f"{which}: statement stop {want[1]}, frozen block-iterations {frozen}, margin {want[5]:.3g}")
    # the binary64 device holds phi to 1e-11 (TOL): a comparison 1e-3 of its tolerance from flipping is five orders away
    assert want[5] >= 1e-3 and (which == "stop_tol" or frozen > 0)
    Ab, Az = transforms(sp, case, "fp64")
    beta, iters, phi, live = sp.amp_sc_batch(y.reshape(1, -1), case.Pl, T, Ab, beta0=b0.reshape(1, -1), return_live=True, **kw)
    assert int(iters[0]) == want[1]
    assert np.array_equal(live[0], want[3])
    assert rel(beta, want[0]) <= TOL["fp64"]
    # the staged run with the same tolerances is the one-call entry point
    op = Ab.op
    op.reserve(1, T)
    op.stage(y.reshape(1, -1), case.Pl, beta0=b0.reshape(1, -1))
    op.run(1, T, beta0=True, **kw)
    op.wait()
    assert np.array_equal(op.fetch_beta(1), beta) and np.array_equal(op.iters(1), iters)


# ---- e. the glue is the uncoupled glue ------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", [jc.K0, jc.K2], ids=lambda c: c.name)  # l0 = 0; l0 = 18 inside a column block
def test_glue_equals_the_uncoupled_glue(sp, case, prec):
    Ab, Az = transforms(sp, case, prec)
    cop = Ab.op
    uop = sp.SparcOperator(case.L, case.M, case.n, case.ordering, "hadamard", prec, 0)
    code = ldpc_code(sp)
    B, L, M, l0, ns, lgm = 3, case.L, case.M, case.l0, case.ns, case.lgm
    rs = np.random.RandomState(23)
    Pl = orc.pa_parameterised(L, 1.0, case.P, 1.0, 0.5)
    beta = np.asarray(go.soft_beta0(np.zeros((B, L * M)), rs.randn(B, L * lgm) * 4, case.n, Pl, L, M, 0, L), dtype=np.float64)
    beta[1] = np.asarray(go.onehot(case.n, Pl, M, rs.randint(0, M, (1, L))), dtype=np.float64)[0]  # decided sections
    ys = rs.randn(B, case.n)
    app = rs.randn(B, ns * lgm) * 5

    def stage():
        uop.reserve(B, 4)
        uop.stage(ys, Pl, beta)
        cop.reserve(B, 4)
        cop.stage(ys, Pl, beta0=beta)

    stage()
    assert np.array_equal(cop.fetch_beta(B), uop.fetch(B)[0])
    d_ch, d_app, _ = code.device_buffers(B)
    for mode, clip in (("reference", None), ("two_sided", None), ("reference", 20.0), ("two_sided", 12.5)):
        a, b = uop.llr(B, l0, ns, mode=mode, clip=clip), cop.llr(B, l0, ns, mode=mode, clip=clip)
        assert a.shape == b.shape == (B, ns * lgm) and np.array_equal(a, b), (mode, clip)
        # SA_PTR_DEVICE: into the LDPC decoder's channel buffer; a run of 0 iterations hands it back as the app
        got = []
        for op in (uop, cop):
            op.llr(B, l0, ns, out=d_ch, mode=mode, clip=clip)
            code.run_buffers(B, max_iter=0)
            got.append(code.fetch_buffers(B)[0])
        assert np.array_equal(got[0], a) and np.array_equal(got[1], a), (mode, clip)
    assert np.array_equal(uop.hard_cancel(B, l0, ns, app), cop.hard_cancel(B, l0, ns, app))
    assert np.array_equal(cop.hard_cancel(B, l0, ns, app), go.hard_indices(app, M))
    uop.soft_beta0(B, l0, ns, app)
    cop.soft_beta0(B, l0, ns, app)
    soft = cop.fetch_beta(B)
    assert np.array_equal(soft, uop.fetch(B)[0]) and not np.array_equal(soft, beta)
    # the same through device pointers: the app of a BP run on the LLRs of the staged beta
    stage()
    cop.llr(B, l0, ns, out=d_ch, clip=30.0)  # (bounded: the decided sections' +-max LLRs would give BP inf - inf)
    code.run_buffers(B, max_iter=3)
    assert np.array_equal(uop.hard_cancel(B, l0, ns, d_app), cop.hard_cancel(B, l0, ns, d_app))
    uop.soft_beta0(B, l0, ns, d_app)
    cop.soft_beta0(B, l0, ns, d_app)
    soft_dev = cop.fetch_beta(B)
    assert np.isfinite(soft_dev).all() and np.array_equal(soft_dev, uop.fetch(B)[0]) and not np.array_equal(soft_dev, soft)
    idx = rs.randint(0, M, (B, L)).astype(np.int32)
    uop.stage_onehot(idx)
    cop.stage_onehot(idx)
    assert np.array_equal(cop.fetch_beta(B), uop.fetch(B)[0])
    assert np.array_equal(cop.decide(B), idx)


# ---- f. forced inputs: every seed, the ones whose BP runs out included --------------------------------
@pytest.mark.parametrize("case,seed,mode", jc.TABLE, ids=lambda v: getattr(v, "name", str(v)))
def test_forced_inputs(sp, case, seed, mode):
    Ab, Az = transforms(sp, case, "fp64")
    op = Ab.op
    r = jc.rep(case, seed, mode)
    L, M, l0, ns = case.L, case.M, case.l0, case.ns
    op.reserve(1, jc.T)
    op.stage_power(1, case.Pl)
    op.encode(r["idx"].reshape(1, -1), r["noise"].reshape(1, -1))
    op.run(1, jc.T)
    op.wait()
    e0 = rel(op.fetch_beta(1), r["betas"][0])
    dec0 = r["betas"][0].reshape(L, M).argmax(axis=1)
    assert e0 <= TOL["fp64"], e0
    assert np.array_equal(op.decide(1)[0], dec0)
    errs = [e0]
    calls = range(len(r["apps"]))
    for k in calls:  # every restart from the statement's own hand-back
        if mode == "soft":
            if k > 0:  # the estimate the statement restarted from
                op.stage(r["y"].reshape(1, -1), beta0=r["betas"][k].reshape(1, -1))
            assert np.array_equal(op.hard_cancel(1, l0, ns, r["apps"][k].reshape(1, -1))[0], r["decs"][k][l0:])
            op.soft_beta0(1, l0, ns, r["apps"][k].reshape(1, -1))
        else:
            op.stage_onehot(r["decs"][k].reshape(1, -1))
        op.run(1, jc.T, beta0=True)
        op.wait()
        e = rel(op.fetch_beta(1), r["betas"][k + 1])
        errs.append(e)
        assert e <= TOL["fp64"], (k, e)
        assert np.array_equal(op.decide(1)[0], r["betas"][k + 1].reshape(L, M).argmax(axis=1))
    print(f"case {case.name} seed {seed} {mode}: beta {' '.join(f'{e:.2e}' for e in errs)}; statement BP {r['bp_iters']}")


# ---- g. the loop ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", jc.MODES)
@pytest.mark.parametrize("case", jc.JOINT_CASES, ids=lambda c: c.name)
def test_joint_decoder_counts_equal_the_statement(sp, case, mode):
    jd = decoder(sp, case)
    assert (jd.l0, jd.ns) == (case.l0, case.ns)
    seeds = case.exact(mode)
    assert seeds
    reps = [jc.rep(case, s, mode) for s in seeds]
    idx = np.stack([r["idx"] for r in reps]).astype(np.int32)
    noise = np.stack([r["noise"] for r in reps])
    out = jd.run(idx, noise, case.Pl, mode, jc.SOFT_ITER)
    for k, (s, r) in enumerate(zip(seeds, reps)):
        got = (list(out["amp"][k]), list(out["ldpc"][k]), list(out["bp_iters"][k]))
        print(f"case {case.name} {mode} seed {s}: amp {got[0]} ldpc {got[1]} bp {got[2]}")
        assert got == (r["amp"], r["ldpc"], r["bp_iters"]), (s, got)


@pytest.mark.parametrize("mode", jc.MODES)
def test_mc_joint_batch_equals_its_reps(sp, mode):
    from sparc_ldpc_amd.joint import mc_joint
    case = jc.K1
    jd = decoder(sp, case)
    seeds = list(jc.SCAN)
    allr = mc_joint(jd, case.Pl, case.sigma, seeds, mode, jc.SOFT_ITER, batch=5)
    for j in (0, 3, 6, 11):
        one = mc_joint(jd, case.Pl, case.sigma, [seeds[j]], mode, jc.SOFT_ITER, batch=1)
        for k in one:
            assert np.array_equal(one[k][0], allr[k][j]), (mode, k, j)
    # and the exact-count reps are the statement's
    for s in case.exact(mode):
        r = jc.rep(case, s, mode)
        j = seeds.index(s)
        assert list(allr["amp"][j]) == r["amp"] and list(allr["ldpc"][j]) == r["ldpc"] and list(allr["bp_iters"][j]) == r["bp_iters"]


# ---- h. reduction to the reference at W = [[1]] -------------------------------------------------------
def _golden_keys():
    g = golden("joint.npz")
    return sorted({k.rsplit("|", 1)[0] for k in g if k.count("|") == 3 and k.split("|")[0] in ("small", "mid", "noisy")
                   and k.split("|")[1] in ("soft", "hard")})


@pytest.mark.parametrize("key", _golden_keys())
def test_flat_base_matrix_meets_the_reference_reps(sp, key):
    from sparc_ldpc_amd.joint import joint_decoder
    G = golden("joint.npz")
    tag, mode, seed = key.split("|")
    L, M, P, r, T, z, sigma = G[f"{tag}|cfg"]
    L, M, T = int(L), int(M), int(T)
    n = int(L * np.log2(M) / r)
    if "flat" not in _JD:
        _JD["flat"] = sp.CoupledJointDecoder(L, M, n, np.ones((1, 1)), ldpc_code(sp), T, device=0)
    jd = _JD["flat"]
    assert (jd.L, jd.M, jd.n, jd.T) == (L, M, n, T)
    np.random.seed(int(seed))
    idx, noise = jd.draw(np.random, 1, float(sigma))
    Pl = float(P) / L * np.ones(L)
    out = jd.run(idx, noise, Pl, mode, 2)
    tb = jd.total_bits
    got = np.array([e / tb for e in out["amp"][0]] + [e / tb for e in out["ldpc"][0]])
    want = G[key + "|ber"]
    its = [int(G[key + f"|it{k}"][0]) for k in range(4) if key + f"|it{k}" in G]
    assert got[0] == want[0]
    if all(i < 200 for i in its):  # test_joint_reps_match_reference's bars
        np.testing.assert_array_equal(got, want)
    else:
        assert np.max(np.abs(got - want)) <= 0.03
    # the same counts as the uncoupled joint decoder on the same draws
    ujd = joint_decoder(L, M, n, sp.LDPCParams("802.16", "5/6", int(z)), T, precision="fp64")
    uout = ujd.run(idx, noise, Pl, mode, 2)
    if all(i < 200 for i in its):
        for k in ("amp", "ldpc", "bp_iters"):
            assert np.array_equal(out[k], uout[k]), k
    else:
        assert out["amp"][0, 0] == uout["amp"][0, 0]


# ---- i. device draws -----------------------------------------------------------------------------------
def test_device_draws(sp):
    from sparc_ldpc_amd.joint import draw_reps, mc_joint
    case = jc.K1
    jd = decoder(sp, case)
    seeds = list(case.exact("soft")) + [6, 7]
    idx_dev = jd.stage_seeds(seeds, case.sigma, case.Pl)
    idx_host, _ = draw_reps(jd.code, case.L, case.M, case.n, [np.random.RandomState(s) for s in seeds], len(seeds), case.sigma)
    assert idx_dev.dtype == np.int32 and np.array_equal(idx_dev, idx_host)
    _, noise_dev = jd.code.joint_fetch()
    for mode in jc.MODES:
        dev = mc_joint(jd, case.Pl, case.sigma, seeds, mode, jc.SOFT_ITER, batch=len(seeds), draws="device")
        host = jd.run(idx_dev, noise_dev, case.Pl, mode, jc.SOFT_ITER)  # a host-drawn run fed the device's noise
        for k in host:
            assert np.array_equal(dev[k], host[k]), (mode, k)


# ---- j. refusals ---------------------------------------------------------------------------------------
def test_refusals_through_the_abi(sp, lib_gpu):
    L_ = sp._lib
    case = jc.K2
    parent = sp.SparcOperator(case.L, case.M, case.n, case.ordering, "hadamard", "fp32", 0)
    op = sp.CoupledOperator(parent, case.W)  # a fresh context: nothing reserved
    sc = op._sc
    msg = lambda: lib_gpu.sa_last_error().decode()
    assert lib_gpu.sa_sc_run(sc, 1, 4, 0.0, 0.0, 0) == L_.SA_ERR_ARG and "reserve" in msg()       # run before reserve
    op.reserve(2, 8)
    assert lib_gpu.sa_sc_run(sc, 1, 4, 0.0, 0.0, 0) == L_.SA_ERR_ARG and "power" in msg()
    op.stage_power(2, case.Pl)
    assert lib_gpu.sa_sc_run(sc, 1, 4, 0.0, 0.0, 0) == L_.SA_ERR_ARG and "nothing staged" in msg()  # run before stage
    ys = np.stack([case.rep(1)[1], case.rep(2)[1]])
    op.stage(ys)
    assert lib_gpu.sa_sc_run(sc, 2, 4, 0.0, 0.0, L_.SA_FLAG_BETA0) == L_.SA_ERR_ARG and "no beta staged" in msg()
    assert lib_gpu.sa_sc_run(sc, 3, 4, 0.0, 0.0, 0) == L_.SA_ERR_ARG
    assert lib_gpu.sa_sc_run(sc, 2, 9, 0.0, 0.0, 0) == L_.SA_ERR_ARG and "T" in msg()
    assert lib_gpu.sa_sc_run(sc, 2, 4, -1.0, 0.0, 0) == L_.SA_ERR_ARG and "stop_tol" in msg()
    assert lib_gpu.sa_sc_run(sc, 2, 4, 0.0, 0.0, 64) == L_.SA_ERR_ARG and "flags" in msg()
    out = np.full((2, case.ns * case.lgm), 7.0)
    assert lib_gpu.sa_sc_llr(sc, 2, case.l0, case.ns, out.ctypes.data_as(ct.c_void_p), 0, 0, float("inf")) == L_.SA_ERR_ARG
    assert "no beta staged" in msg()
    op.run(2, 4)
    op.wait()
    want = op.fetch_beta(2)
    i32 = ct.POINTER(ct.c_int32)
    idx = np.full((2, case.ns), -5, dtype=np.int32)
    app = np.zeros((2, case.ns * case.lgm))
    for l0, ns in ((-1, 4), (0, 0), (case.l0, case.ns + 1), (case.L, 1)):  # bad l0 / ns
        assert lib_gpu.sa_sc_llr(sc, 2, l0, ns, out.ctypes.data_as(ct.c_void_p), 0, 0, float("inf")) == L_.SA_ERR_ARG
        assert lib_gpu.sa_sc_soft_beta0(sc, 2, l0, ns, app.ctypes.data_as(ct.c_void_p), 0) == L_.SA_ERR_ARG
        assert lib_gpu.sa_sc_hard_indices(sc, 2, l0, ns, app.ctypes.data_as(ct.c_void_p), 0, idx.ctypes.data_as(i32)) == L_.SA_ERR_ARG
    assert lib_gpu.sa_sc_llr(sc, 2, case.l0, case.ns, out.ctypes.data_as(ct.c_void_p), 0, 5, float("inf")) == L_.SA_ERR_ARG
    bad = np.zeros((2, case.L), dtype=np.int32)
    bad[1, 3] = case.M
    assert lib_gpu.sa_sc_stage_onehot(sc, 2, bad.ctypes.data_as(i32)) == L_.SA_ERR_ARG and "index" in msg()
    assert lib_gpu.sa_sc_encode(sc, 2, bad.ctypes.data_as(i32), None) == L_.SA_ERR_ARG
    # outputs and the stage are untouched: the same run gives the same estimate
    assert (out == 7.0).all() and (idx == -5).all()
    assert np.array_equal(op.fetch_beta(2), want)
    op.run(2, 4)
    op.wait()
    assert np.array_equal(op.fetch_beta(2), want)
    # a one-call entry point overwrites the workspace: nothing is staged after it
    op.amp_batch(ys, case.Pl, 2)
    assert lib_gpu.sa_sc_run(sc, 2, 4, 0.0, 0.0, 0) == L_.SA_ERR_ARG and "nothing staged" in msg()
    op.Ab_batch(np.zeros((1, case.L * case.M)))
    op.stage(ys)
    op.Az_batch(np.zeros((1, case.n)))
    with pytest.raises(sp.SparcAmpArgumentError, match="nothing staged"):
        op.run(2, 4)
    assert lib_gpu.sa_sc_run(None, 1, 1, 0.0, 0.0, 0) == L_.SA_ERR_ARG
    assert lib_gpu.sa_sc_amp_start(sc, 1, ys.ctypes.data_as(D), case.Pl.ctypes.data_as(D), 2, None, 0.0, 0.0, None, None, None,
                                   None, 0) == L_.SA_ERR_ARG


def test_refusals_of_the_joint_decoder(sp):
    from sparc_ldpc_amd.joint import mc_joint
    case = jc.K1
    jd = decoder(sp, case)
    r = jc.rep(case, case.exact("soft")[0], "soft")
    idx, noise = r["idx"].reshape(1, -1), r["noise"].reshape(1, -1)
    for mode in ("originalHard", "threshold"):
        with pytest.raises(ValueError, match="shortened / masked"):
            jd.run(idx, noise, case.Pl, mode)
        with pytest.raises(ValueError, match="shortened / masked"):
            mc_joint(jd, case.Pl, case.sigma, [1], mode)
        with pytest.raises(ValueError, match="shortened / masked"):
            mc_joint(jd, case.Pl, case.sigma, [1], mode, draws="device")
    with pytest.raises(ValueError):
        jd.run(idx, noise, case.Pl, "nonsense")
    with pytest.raises(ValueError, match="pipeline"):
        mc_joint(jd, case.Pl, case.sigma, [1, 2], "soft", pipeline=True)
    # the default never pipelines a coupled decoder, whatever the batch
    out = mc_joint(jd, case.Pl, case.sigma, list(range(1, 3)) * 40, "hard", batch=80)
    assert out["amp"].shape == (80, 2) and jd._pipeline is None
    with pytest.raises(ValueError):
        sp.CoupledJointDecoder(case.L, case.M, case.n, case.W, ldpc_code(sp), jc.T, device=0, llr="nonsense")


def test_joint_options_and_tolerances_are_honoured(sp):
    case = jc.K1
    s = case.exact("soft")[0]
    r = jc.rep(case, s, "soft")
    idx, noise = r["idx"].reshape(1, -1).astype(np.int32), r["noise"].reshape(1, -1)
    base = decoder(sp, case).run(idx, noise, case.Pl, "soft", 2)
    jd = sp.CoupledJointDecoder(case.L, case.M, case.n, case.W, ldpc_code(sp), jc.T, device=0, llr="two_sided", llr_clip=25.0,
                                bp_dectype="minsum", bp_max_iter=50, stop_tol=1e-3, freeze_tol=1e-2)
    assert jd.options["llr"] == "two_sided" and jd.options["bp_dectype"] == "minsum" and jd.op is not jd.coupled
    out = jd.run(idx, noise, case.Pl, "soft", 2)
    assert out["amp"].shape == base["amp"].shape and out["amp"][0, 0] == base["amp"][0, 0]
    assert (out["bp_iters"] <= 50).all()
    assert jd.coupled.iters(1)[0] <= jc.T
