"""GPU: sa_llr_ex (the two-sided, clipped section->bit LLR) against its NumPy
statement (tests/joint_llr_ref.py), and the LLR / BP options of the joint
decoder against the same stages called one by one.

Bounds (ε = 2^-52): where p0, p1 > 0 the device and the statement form the same
ordered binary64 sums, so |got − ref| <= 64 ε (|log p0| + |log p1|), the two
device logarithms; saturated and clipped values are exact.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np
import pytest

import joint_llr_ref as jr
from oracle import glue_oracle as go

pytestmark = pytest.mark.gpu

F64_MAX = jr.F64_MAX
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


_OPS = {}


def operator(sp, L, M, n, prec):
    key = (L, M, n, prec)
    if key not in _OPS:
        op = sp.SparcOperator(L, M, n, sp.make_ordering(L, M, n), precision=prec)
        op.reserve(3, 1)
        op.stage_power(3, jr.power(L))
        _OPS[key] = op
    return _OPS[key]


@pytest.fixture(scope="module", autouse=True)
def release():
    yield
    _OPS.clear()
    _JDS.clear()


def stage(op, beta, prec):
    """Stage β and return it as the device holds it (op.fetch)."""
    B = beta.shape[0]
    op.stage(np.zeros((B, op.n)), jr.power(op.L), beta)
    got = op.fetch(B)[0]
    assert np.array_equal(got, jr.held(beta, prec))
    return got


def llr_ex(op, B, l0, ns, mode, clip, out=None):
    """sa_llr_ex itself -> (status, the output array)."""
    lgm = int(np.log2(op.M))
    if out is None:
        out = np.full((B, ns * lgm), SENTINEL)
    rc = op._lib.sa_llr_ex(op.ctx, B, l0, ns, ct.c_void_p(out.ctypes.data), 0, int(mode), float(clip))
    return rc, out


# ---- 1. the reference mode is sa_llr ----------------------------------------------------

@pytest.mark.parametrize("prec", jr.PRECS)
@pytest.mark.parametrize("geom,rng", jr.RANGED, ids=jr.RANGED_IDS)
def test_reference_mode_is_sa_llr(sp, geom, rng, prec):
    L, M, n, B, _ = geom
    l0, ns = rng
    op = operator(sp, L, M, n, prec)
    hand = jr.hand_vectors(B, L, M, n, jr.power(L))[0]
    for beta in (jr.draw(M, B, L, n, jr.LLR_SCALE[M]), jr.draw(M, B, L, n, jr.WIDE_SCALE), hand):
        stage(op, beta, prec)
        want = op.llr(B, l0, ns)
        for clip in (np.inf, 0.0):
            rc, got = llr_ex(op, B, l0, ns, 0, clip)
            assert rc == 0 and np.array_equal(got, want)
        assert np.array_equal(op.llr(B, l0, ns, mode="reference", clip=None), want)
        # the clip in mode 0: np.clip of sa_llr's output, 0 staying 0
        for clip in (20.0, 0.5):
            got = op.llr(B, l0, ns, clip=clip)
            assert np.array_equal(got, np.clip(want, -clip, clip))
            assert np.array_equal(got == 0.0, want == 0.0)


# ---- 2. the two-sided mode against the statement ------------------------------------------

@pytest.mark.parametrize("scale", ["regular", "wide"])
@pytest.mark.parametrize("prec", jr.PRECS)
@pytest.mark.parametrize("geom,rng", jr.RANGED, ids=jr.RANGED_IDS)
def test_two_sided_against_the_statement(sp, geom, rng, prec, scale):
    L, M, n, B, _ = geom
    l0, ns = rng
    op, Pl = operator(sp, L, M, n, prec), jr.power(L)
    beta = stage(op, jr.draw(M, B, L, n, jr.LLR_SCALE[M] if scale == "regular" else jr.WIDE_SCALE), prec)
    ref, p0, p1 = jr.two_sided_llr(beta, n, Pl, L, M, l0, ns, prec)
    assert p0.min() > 0 and p1.min() > 0, "precondition: both sums positive"
    got = op.llr(B, l0, ns, mode="two_sided")
    assert got.shape == ref.shape
    err = np.abs(np.asarray(go.LD(1) * got - ref, dtype=np.float64))
    bound = jr.log_bound(p0, p1)
    print(f"llr2 M={M} {prec} {scale}: max |llr| {np.abs(got).max():.1f}, max err {err.max():.2e}, "
          f"worst err/bound {(err / bound).max():.3f}")
    assert np.all(err <= bound)
    # clipped: the statement's clip of the same values
    lim = 0.25 * float(np.abs(got).max())
    refc = np.asarray(jr.two_sided_llr(beta, n, Pl, L, M, l0, ns, prec, lim)[0], dtype=np.float64)
    gotc = op.llr(B, l0, ns, mode="two_sided", clip=lim)
    assert np.abs(gotc).max() == lim and np.all(np.abs(gotc - refc) <= bound)
    assert np.array_equal(gotc, np.clip(got, -lim, lim))


# ---- 3. saturated vectors ---------------------------------------------------------------------

@pytest.mark.parametrize("prec", jr.PRECS)
@pytest.mark.parametrize("geom,rng", jr.RANGED, ids=jr.RANGED_IDS)
def test_two_sided_saturated(sp, geom, rng, prec):
    """One-hot, empty and overfull sections: ∓max on the set / clear bits, 0 on
    an empty section (the reference form: +max), no NaN -> 0 on an overfull one."""
    L, M, n, B, _ = geom
    l0, ns = rng
    lgm = int(np.log2(M))
    op = operator(sp, L, M, n, prec)
    beta, sign = jr.hand_vectors(B, L, M, n, jr.power(L))
    stage(op, beta, prec)
    sign = sign.reshape(B, L, lgm)[:, l0:l0 + ns].reshape(B, ns * lgm)
    for clip, mag in ((None, F64_MAX), (0.0, F64_MAX), (np.inf, F64_MAX), (20.0, 20.0), (0.5, 0.5)):
        got = op.llr(B, l0, ns, mode="two_sided", clip=clip)
        assert np.array_equal(got, sign * mag), clip
        assert not np.signbit(got[got == 0.0]).any()


# ---- 4. device-pointer output --------------------------------------------------------------------

@pytest.mark.parametrize("prec", jr.PRECS)
def test_device_pointer_output(sp, prec):
    L, M, n, l0, ns, B = 64, 16, 256, 16, 48, 2
    code = sp.code("802.16", "5/6", 8)
    d_ch, d_app, _ = code.device_buffers(B)
    op = operator(sp, L, M, n, prec)
    stage(op, jr.soft_beta(np.random.RandomState(7), B, L, M, n, jr.power(L), 12.0), prec)
    for mode, clip in (("two_sided", None), ("two_sided", 9.0), ("reference", 9.0)):
        host = op.llr(B, l0, ns, mode=mode, clip=clip)
        assert np.isfinite(host).all() and (clip is None or np.abs(host).max() == clip)
        op.llr(B, l0, ns, out=d_app, mode=mode, clip=clip)  # lands where fetch_buffers reads
        assert np.array_equal(code.fetch_buffers(B)[0], host)


# ---- 5. refusals -------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", jr.PRECS)
def test_refusals_write_nothing(sp, prec):
    L, M, n, B, _ = jr.GEOMS[0]
    op = operator(sp, L, M, n, prec)
    beta = stage(op, jr.draw(M, B, L, n, 3.0), prec)
    for mode, clip in ((2, np.inf), (-1, np.inf), (1, -1.0), (0, -1.0), (1, np.nan), (0, np.nan), (1, -np.inf)):
        rc, out = llr_ex(op, B, 2, 4, mode, clip)
        assert rc == -1, (mode, clip)  # SA_ERR_ARG
        assert np.all(out == SENTINEL)
        assert np.array_equal(op.fetch(B)[0], beta)
    for clip in (-1.0, np.nan):
        with pytest.raises(sp.SparcAmpError):
            op.llr(B, 2, 4, mode="two_sided", clip=clip)
    with pytest.raises(ValueError):
        op.llr(B, 2, 4, mode="both")
    rc, out = llr_ex(op, B, 2, 4, 1, np.inf)  # and the call still works
    assert rc == 0 and np.all(out != SENTINEL)


# ---- 6. the joint decoder's options: the same stages one by one ------------------------------------------

SHAPE = dict(L=64, M=16, n=256, z=8, T=30, P=4.0, sigma=0.93, seeds=range(500, 508))
OPTION_SETS = {
    "two_sided-clip25-layered_minsum_f32": dict(llr="two_sided", llr_clip=25.0, bp_dectype="layered_minsum_f32"),
    "reference-layered_sumprod2": dict(llr="reference", llr_clip=None, bp_dectype="layered_sumprod2"),
    "two_sided-clip25-layered_minsum-quant": dict(llr="two_sided", llr_clip=25.0, bp_dectype="layered_minsum",
                                                  bp_quant=True),
}
_JDS = {}


def decoder(sp, name, prec="fp64"):
    from sparc_ldpc_amd import joint
    if (name, prec) not in _JDS:
        s = SHAPE
        code = sp.code("802.16", "5/6", s["z"])
        _JDS[(name, prec)] = joint.JointDecoder(s["L"], s["M"], s["n"], code, s["T"], precision=prec,
                                                **OPTION_SETS[name])
    return _JDS[(name, prec)]


def reps(jd, sigma):
    return jd.draw([np.random.RandomState(s) for s in SHAPE["seeds"]], len(SHAPE["seeds"]), sigma)


def composed(jd, idx, noise, Pl, mode, o, soft_iter=2, threshold=0.5):
    """The joint schemes (joint.py's module docstring) written out stage by stage with the options o."""
    op, code, sub = jd.op, jd.code, jd.sub
    L, logm, l0, ns, T, B = jd.L, jd.logm, jd.l0, jd.ns, jd.T, idx.shape[0]
    llr_kw = dict(mode=o["llr"], clip=o["llr_clip"])
    bp_kw = dict(dectype=o["bp_dectype"], quant=o.get("bp_quant"))
    jd.stage(idx, noise, Pl)
    op.run(B, T)
    op.wait()
    rx = op.decide(B)
    amp, ldpc, iters, out = [jd._errs(idx, rx)], [], [], {}

    def bp():
        d_ch, d_app, _ = code.device_buffers(B)
        op.llr(B, l0, ns, out=d_ch, **llr_kw)
        code.run_buffers(B, **bp_kw)
        iters.append(code.fetch_buffers(B, app=False)[1])
        dec = rx.copy()
        dec[:, l0:] = op.hard_cancel(B, l0, ns, d_app, dst=sub if mode == "originalHard" else None)
        ldpc.append(jd._errs(idx, dec))
        return d_app, dec

    if mode == "originalHard":
        _, dec = bp()
        sub.stage_power(B, Pl[:l0])
        sub.run(B, T)
        sub.wait()
        dec[:, :l0] = sub.decide(B)
        out["ldpc_amp"] = jd._errs(idx, dec)
    elif mode == "soft":
        for _ in range(soft_iter):
            d_app, _ = bp()
            op.soft_beta0(B, l0, ns, d_app)
            op.run(B, T, beta0=True)
            op.wait()
            rx = op.decide(B)
            amp.append(jd._errs(idx, rx))
    elif mode == "hard":
        _, dec = bp()
        op.stage_onehot(dec)
        op.run(B, T, beta0=True)
        op.wait()
        amp.append(jd._errs(idx, op.decide(B)))
    else:  # threshold
        LLR = op.llr(B, 0, L, **llr_kw)
        mk = op.subset(np.arange(L))
        mk.reserve(B, T)
        mk.stage_power(B, Pl)
        for i in range(soft_iter):
            app, it = code.decode_batch(LLR[:, l0 * logm:], **bp_kw)
            iters.append(it)
            LLR[:, l0 * logm:] = app
            ldpc.append(jd._llr_errs(idx, LLR))
            if i == soft_iter - 1:
                break
            full = np.full((B, L), -1, dtype=np.int32)
            full[:, l0:] = op.threshold(B, l0, ns, app, threshold)
            und = full < 0
            if und.any():
                op.cancel(full, mk)
                mk.stage_power_batch(B, np.where(und, Pl[None, :], 0.0))
                mk.run(B, T)
                mk.wait()
                LLR.reshape(B, L, logm)[und] = mk.llr(B, 0, L, **llr_kw).reshape(B, L, logm)[und]
            amp.append(jd._llr_errs(idx, LLR))
    out.update(amp=np.stack(amp, axis=1), ldpc=np.stack(ldpc, axis=1), bp_iters=np.stack(iters, axis=1))
    return out


@pytest.mark.parametrize("mode", ["soft", "originalHard", "hard", "threshold"])
@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_run_with_options_is_the_stages_one_by_one(sp, name, mode):
    from sparc_ldpc_amd import joint
    jd = decoder(sp, name)
    o = OPTION_SETS[name]
    assert jd.options == joint.joint_options(**o) and jd.options != joint.joint_options()
    Pl = SHAPE["P"] / SHAPE["L"] * np.ones(SHAPE["L"])
    idx, noise = reps(jd, SHAPE["sigma"])
    got = jd.run(idx, noise, Pl, mode)
    want = composed(jd, idx, noise, Pl, mode, o)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert got["bp_iters"].min() >= 0 and got["ldpc"].shape[1] >= 1
    print(f"{name} {mode}: amp {got['amp'].sum(axis=0).tolist()} ldpc {got['ldpc'].sum(axis=0).tolist()} "
          f"bp sweeps {got['bp_iters'].mean(axis=0).round(1).tolist()}")


@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_options_key_the_decoder_cache(sp, name):
    """joint_decoder keeps a decoder per option set; the first AMP takes no option."""
    from sparc_ldpc_amd import joint
    s = SHAPE
    jd = decoder(sp, name)
    plain = joint.joint_decoder(s["L"], s["M"], s["n"], sp.LDPCParams("802.16", "5/6", s["z"]), s["T"])
    assert plain.options == joint.joint_options()
    assert plain is not joint.joint_decoder(s["L"], s["M"], s["n"], sp.LDPCParams("802.16", "5/6", s["z"]), s["T"],
                                            **OPTION_SETS[name])
    Pl = s["P"] / s["L"] * np.ones(s["L"])
    idx, noise = reps(jd, s["sigma"])
    a, b = jd.run(idx, noise, Pl, "soft"), plain.run(idx, noise, Pl, "soft")
    assert np.array_equal(a["amp"][:, 0], b["amp"][:, 0])
    print(f"{name}: bp_iters {a['bp_iters'].mean(axis=0).tolist()} against sumprod2's {b['bp_iters'].mean(axis=0).tolist()}")


def test_pipeline_slices_inherit_the_options(sp):
    from sparc_ldpc_amd import joint
    name = "two_sided-clip25-layered_minsum_f32"
    jd = decoder(sp, name)
    Pl = SHAPE["P"] / SHAPE["L"] * np.ones(SHAPE["L"])
    idx, noise = reps(jd, SHAPE["sigma"])
    one = jd.run(idx, noise, Pl, "soft")
    pipe = joint.joint_pipeline(jd, 2)
    try:
        assert len(pipe.parts) == 2 and all(p.options == jd.options for p in pipe.parts)
        two = pipe.run(idx, noise, Pl, "soft")
    finally:
        joint._evict(jd)
    for k in one:
        assert np.array_equal(one[k], two[k]), k
    # and through mc_joint, which is given the decoder
    three = joint.mc_joint(jd, Pl, SHAPE["sigma"], SHAPE["seeds"], "soft", batch=8, pipeline=False)
    for k in one:
        assert np.array_equal(one[k], three[k]), k


# ---- 7. binary32 end to end ---------------------------------------------------------------------------------

E2E_SIGMA = 0.5


def test_binary32_beta_after_amp(sp):
    """After the first binary32 AMP at sigma = 0.5 (sections decided): the
    one-sided LLR of the β the device holds has exact zeros on bits the
    two-sided statement puts beyond 16; the device's two-sided LLR of the same
    β matches the statement and has no exact zero."""
    jd = decoder(sp, "two_sided-clip25-layered_minsum_f32", "fp32")
    L, M, n, l0, ns, T = jd.L, jd.M, jd.n, jd.l0, jd.ns, jd.T
    Pl = SHAPE["P"] / L * np.ones(L)
    idx, noise = reps(jd, E2E_SIGMA)
    B = idx.shape[0]
    jd.stage(idx, noise, Pl)
    jd.op.run(B, T)
    jd.op.wait()
    beta = jd.op.fetch(B)[0]
    one = np.asarray(go.llr(beta, n, Pl, L, M, l0, ns)[0], dtype=np.float64)
    ref, p0, p1 = jr.two_sided_llr(beta, n, Pl, L, M, l0, ns, "fp32")
    ref64 = np.asarray(ref, dtype=np.float64)
    erased = (one == 0.0) & (np.abs(ref64) > 16)
    both = (p0 > 0) & (p1 > 0)
    print(f"sigma {E2E_SIGMA}: {int(erased.sum())} of {one.size} bits erased by the one-sided form; "
          f"{int((~both).sum())} saturated; max finite |two-sided| {np.abs(ref64[both]).max():.1f}")
    assert erased.any(), "precondition: the one-sided form erases a confident bit"
    got = jd.op.llr(B, l0, ns, mode="two_sided")
    err = np.abs(np.asarray(go.LD(1) * got - ref, dtype=np.float64))
    assert np.all(err[both] <= jr.log_bound(p0, p1)[both])
    assert np.array_equal(got[~both], ref64[~both])
    assert not (got == 0.0).any()
    # the decoder's own call: the same values, clipped
    assert np.array_equal(jd.op.llr(B, l0, ns, **jd._llr_kw), np.clip(got, -25.0, 25.0))


# ---- 8. the per-rep simulators pass the options through ---------------------------------------------------------

def test_per_rep_simulators_take_the_options(sp):
    """One rep of each simulator from the seeded global stream with options: the counts of
    JointDecoder.run on the same draws with the same options (the threshold one, which decodes
    through a shortened operator: its first AMP, and as many rounds)."""
    from sparc_ldpc_amd import joint
    s = SHAPE
    o = OPTION_SETS["two_sided-clip25-layered_minsum_f32"]
    spp = sp.SPARCParams(s["L"], s["M"], s["sigma"], s["P"], 1.0, s["T"])
    lp = sp.LDPCParams("802.16", "5/6", s["z"])
    jd = joint.joint_decoder(s["L"], s["M"], s["n"], lp, s["T"], **o)
    assert jd.options == joint.joint_options(**o)
    Pl = s["P"] / s["L"] * np.ones(s["L"])
    tb = jd.total_bits

    def want(mode):
        np.random.seed(11)
        idx, noise = jd.draw(np.random, 1, s["sigma"])
        return jd.run(idx, noise, Pl, mode)

    np.random.seed(11)
    ba, bl, bla, _ = sp.amp_ldpc_sim(spp, lp, **o)
    r = want("originalHard")
    assert [ba, bl, bla] == [r["amp"][0, 0] / tb, r["ldpc"][0, 0] / tb, r["ldpc_amp"][0] / tb]
    np.random.seed(11)
    ba, bl, _ = sp.soft_amp_ldpc_sim(spp, lp, 2, **o)
    r = want("soft")
    assert ba == [e / tb for e in r["amp"][0]] and bl == [e / tb for e in r["ldpc"][0]]
    np.random.seed(11)
    ba, bl, _ = sp.hardinitbeta_amp_ldpc_sim(spp, lp, **o)
    r = want("hard")
    assert ba == [e / tb for e in r["amp"][0]] and bl == [e / tb for e in r["ldpc"][0]]
    np.random.seed(11)
    ba, bl, _ = sp.soft_amp_ldpc_hardinit(spp, lp, 2, 0.5, **o)
    r = want("threshold")
    assert ba[0] == r["amp"][0, 0] / tb and (len(ba), len(bl)) == (r["amp"].shape[1], r["ldpc"].shape[1])
    with pytest.raises(ValueError):
        sp.soft_amp_ldpc_hardinit(spp, lp, 2, 0.5, llr="both")
    with pytest.raises(TypeError):
        sp.amp_ldpc_sim(spp, llr="two_sided")  # plain SPARC has no LLR
