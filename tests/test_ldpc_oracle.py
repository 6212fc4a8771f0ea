"""CPU: the LDPC oracle against the reference's own fixtures (tests/golden/ldpc.npz,
captured from ldpc/py/ldpc.py and the reference C decoder) and, when built by
oracle/Makefile, against oracle/_ref/c_ldpc.so itself."""
import ctypes as ct
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden
from oracle import ldpc_oracle as lo

REF_SO = os.path.join(ROOT, "oracle", "_ref", "c_ldpc.so")


def _meta():
    with open(os.path.join(GOLDEN, "ldpc_meta.json")) as fh:
        return json.load(fh)


def _key(k):
    std, rate, z, ptype = k.split("|")
    return std, rate, int(z), ptype


def _sha(*arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a, dtype=np.int64).tobytes())
    return h.hexdigest()


def test_graphs_match_reference_prepare_decoder():
    g = golden("ldpc.npz")
    for key, info in _meta()["graphs"].items():
        std, rate, z, ptype = _key(key)
        proto = lo.protograph(std, rate, z, ptype)
        vdeg, cdeg, il = lo.prepare_decoder(proto, z)
        assert _sha(vdeg, cdeg, il) == info["sha"], key
        assert len(vdeg) == info["N"] and len(vdeg) - len(cdeg) == info["K"] and len(il) == info["Nmsg"]
        if z == 3:
            assert np.array_equal(il, g[f"graph|{key}|intrlv"])


@pytest.mark.parametrize("key", ["802.16|1/2|3|A", "802.16|2/3|3|B", "802.11n|3/4|27|A", "802.16|5/6|3|A"])
def test_pcmat_degrees(key):
    std, rate, z, ptype = _key(key)
    proto = lo.protograph(std, rate, z, ptype)
    H = lo.pcmat(proto, z)
    vdeg, cdeg, il = lo.prepare_decoder(proto, z)
    assert H.sum() == len(il) and np.array_equal(H.sum(0), vdeg) and np.array_equal(H.sum(1), cdeg)


def test_encoder_kats():
    g = golden("ldpc.npz")
    meta = _meta()
    for key in meta["encode_codes"]:
        std, rate, z, ptype = _key(key)
        proto = lo.protograph(std, rate, z, ptype)
        H = lo.pcmat(proto, z) if z <= 54 else None
        for u, x in zip(g[f"enc|{key}|info"], g[f"enc|{key}|code"]):
            got = lo.encode(proto, z, u)
            assert np.array_equal(got, x), key
            if H is not None:
                assert not np.any(H.dot(got) % 2)
    for key in meta["encode_raises"]:
        std, rate, z, ptype = _key(key)
        proto = lo.protograph(std, rate, z, ptype)
        with pytest.raises(NameError):
            lo.encode(proto, z, np.zeros((proto.shape[1] - proto.shape[0]) * z, dtype=int))


def _decode_cases():
    return _meta()["decode_cases"]


@pytest.mark.parametrize("tag", _decode_cases())
def test_decoder_kats(tag):
    g = golden("ldpc.npz")
    parts = tag.split("|")
    std, rate, z, ptype, algo = parts[1], parts[2], int(parts[3]), parts[4], parts[-1]
    proto = lo.protograph(std, rate, z, ptype)
    vdeg, cdeg, il = lo.prepare_decoder(proto, z)
    ch = g[tag + "|ch"]
    ref_app, ref_it = g[tag + "|app"], int(g[tag + "|it"][0])
    app, it = lo._decode(ch, vdeg, cdeg, il, algo)
    assert it == ref_it
    if ref_it < lo.MAX_ITCOUNT:
        # converged decodes: NumPy vs glibc exp/log differ by ulps at most
        assert np.array_equal(app < 0, ref_app < 0)
        # tanh/atanh (sumprod) is ill-conditioned near +-1 and amplifies ulps more
        tol = 1e-3 if algo == "sumprod" else 1e-9
        np.testing.assert_allclose(app, ref_app, rtol=tol, atol=tol)
    else:
        # 200 non-converging iterations amplify ulp differences; decisions stay close
        assert np.mean((app < 0) != (ref_app < 0)) < 0.02


def _ref_lib():
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref/c_ldpc.so not built (make -C oracle; needs /root/reference)")
    lib = ct.CDLL(REF_SO)
    lib.Lxor.restype = ct.c_double
    lib.Lxor.argtypes = [ct.c_double, ct.c_double, ct.c_int]
    lib.Lxfb.restype = ct.c_double
    lib.Lxfb.argtypes = [ct.POINTER(ct.c_double), ct.c_long, ct.c_int]
    return lib


def test_lxor_lxfb_against_reference_c():
    lib = _ref_lib()
    rs = np.random.RandomState(3)
    a = rs.randn(200) * 5
    b = rs.randn(200) * 5
    a[:5] = [0.0, -0.0, 1e300, -1e308, 40.0]
    for corr in (0, 1):
        ref = np.array([lib.Lxor(x, y, corr) for x, y in zip(a, b)])
        np.testing.assert_allclose(lo.lxor(a, b, bool(corr)), ref, rtol=1e-14, atol=1e-15)
    for dc in (2, 3, 7, 20, 25):
        L = rs.randn(dc) * 3
        Lr = L.copy()
        agg_ref = lib.Lxfb(Lr.ctypes.data_as(ct.POINTER(ct.c_double)), dc, 1)
        Lm = L[None, :].copy()
        agg = lo.lxfb(Lm, True)
        np.testing.assert_allclose(Lm[0], Lr, rtol=1e-13, atol=1e-14)
        assert abs(agg[0] - agg_ref) <= 1e-13 * max(1, abs(agg_ref))


def test_sp2bp_bp2sp_llr_against_reference():
    g = golden("ldpc.npz")
    for L, M in ((6, 8), (4, 64), (3, 512)):
        beta = g[f"sp2bp|{L}|{M}|beta"]
        p = lo.sp2bp(beta, L, M)
        assert np.array_equal(p, g[f"sp2bp|{L}|{M}|p"])
        with np.errstate(divide="ignore"):
            llr = np.nan_to_num(np.log(1 - p) - np.log(p))
        assert np.array_equal(llr, g[f"sp2bp|{L}|{M}|llr"])
        if M <= 64:
            np.testing.assert_allclose(lo.bp2sp(g[f"bp2sp|{L}|{M}|v"], L, M), g[f"bp2sp|{L}|{M}|sp"],
                                       rtol=1e-14, atol=0)


# ---- traced / truncated decodes, Lxor in long double, synthetic graphs -----------------
import ldpc_cases as lc  # noqa: E402


@pytest.mark.parametrize("algo", lc.ALGOS)
@pytest.mark.parametrize("cell", ["16_1/2_z24", "16_5/6_z24", "syn_dc8"])
def test_trace_equals_separate_truncated_runs(cell, algo):
    """One traced run to 12 iterations gives the decode cut at every k <= 12, bit for bit."""
    ref = lc.reference(cell, algo)
    c = ref.c
    fn = {"sumprod2": lo.sumprod2, "sumprod": lo.sumprod, "minsum": lo.minsum}[algo]
    for i, ch in enumerate(ref.CH):
        assert len(ref.apps[i]) == len(ref.margins[i]) == min(ref.its[i] + 1, lc.K_TRACE)
        for k in range(lc.K_TRACE + 1):
            app, it = fn(ch, c.vdeg, c.cdeg, c.intrlv, max_it=k)
            tapp, tit = lo.truncated(ch, ref.its[i], ref.apps[i], k)
            assert it == tit and np.array_equal(app, tapp, equal_nan=True), (ref.labels[i], k)
            if k == 0:
                assert it == 0 and np.array_equal(app, ch) and app is not ch


@pytest.mark.parametrize("cell", list(lc.CELLS))
def test_case_words_meet_their_preconditions(cell):
    """What the GPU trajectory tests assume of their inputs, from the oracle alone."""
    for algo in lc.ALGOS:
        ref = lc.reference(cell, algo)
        ref.check_preconditions(cell, algo)
        assert len(ref.CH) == (2 if cell in lc.TWO_WORDS else 6 if algo == "sumprod" else 8)


def test_lxor_float64_against_long_double():
    a, b = lc.lxor_points()
    assert 1200 <= len(a) <= 1800
    ref = lo.lxor_ld(a, b)
    err = np.abs(lo.lxor(a, b).astype(np.longdouble) - ref).astype(np.float64)
    worst = np.max(err / lc.lxor_bar(a, b)) * 4
    print(f"float64 lxor: worst error {worst:.3f} * 2^-52 * max(1, min(|a|, |b|))")
    assert np.all(err <= lc.lxor_bar(a, b)), worst
    # the edges are in the set: the branch switch, a = +-b, zeros, 1 + exp(-x) == 1, exp underflow
    s, d = np.abs(a + b), np.abs(a - b)
    assert (s == lc.LN_SW).any() and (d == lc.LN_SW).any() and (a == b).any() and (a == -b).any()
    assert ((a == 0) & np.signbit(a)).any() and ((b == 0) & ~np.signbit(b)).any()
    assert (np.abs(s - 37.0) < 1e-9).any() and (np.abs(d - 750.0) < 1e-9).any()
    assert ((a != 0) & (np.abs(a) < 2.3e-308)).any()


@pytest.mark.parametrize("name", list(lc.SYNTH))
def test_synthetic_graphs_product_against_oracle(name):
    from sparc_ldpc_amd import ldpc
    rw, ncols, heavy, _ = lc.SYNTH[name]
    proto = lc.synth_proto(name)
    assert np.array_equal(proto, lc.synth_proto(name))  # seeded
    assert proto.shape == (len(rw), ncols) and (proto < lc.SYNTH_Z).all()
    assert np.array_equal((proto != -1).sum(1), rw) and (proto != -1).any(0).all()
    if heavy:
        assert (proto[:, heavy[0]] != -1).sum() == heavy[1] == 13
    got = ldpc.tanner_graph(proto, lc.SYNTH_Z)
    want = lo.prepare_decoder(proto, lc.SYNTH_Z)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    c = lc.make_code("syn_" + name)
    assert np.array_equal(c.proto, proto) and np.array_equal(c.intrlv, want[2]) and c.cdeg.max() == max(rw)
    H = lo.pcmat(proto, lc.SYNTH_Z)
    assert np.array_equal(H.sum(0), c.vdeg) and np.array_equal(H.sum(1), c.cdeg)
