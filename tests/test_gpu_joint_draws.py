"""GPU: the reps of the joint SPARC + LDPC simulators drawn, LDPC-encoded, packed
and encoded on the device from their seeds (draws="device": lb_joint_draw,
sa_encode_bits) against NumPy (JointDecoder.draw), and the decodes on them
against the decodes of the same arrays fetched back and staged from the host.

Bars.  The message (bits, section indices) is integer work: equality.  The
noise: the bar tests/test_gpu_mc_draws.py derives for randn * sigma on the
device, 2**-49 relative (the device library's log against the C library's,
each within an ulp, and the roundings behind them: <= 4.5 * 2**-52); a
misaligned accept sequence or a wrong start word shows as differences of order
1.  The staged y and every decode result: a fetched-and-restaged batch is the
same computation by the same kernels, so equality.

Shapes (T = 30, uniform Pl = 4 / L, 802.16 rate 5/6):
  A  L=64  M=16 n=256 z=8   K=160 N=192 U=64   (tests/test_gpu_joint.py's shape)
  B  L=192 M=16 n=384 z=24  K=480 N=576 U=192  K + U = 672 > 624: the second
     randint and the start of randn cross an MT output block
  C  L=48  M=16 n=191 z=8   U=0: no second randint, no shortened operator; n odd:
     the last polar pair's partner is dropped
"""
import ctypes as ct
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 2.0 ** -49  # tests/test_gpu_mc_draws.py: BAR, derived there
SEEDS = [0, 1, 2 ** 31, 2 ** 32 - 1] + list(range(1000, 1007))
SEEDS37 = list(range(100, 137))
T = 30
SHAPES = {"A": (64, 16, 256, 8), "B": (192, 16, 384, 24), "C": (48, 16, 191, 8)}  # L, M, n, z
SIGMA = {"A": 0.93, "B": 0.93}  # A: tests/test_gpu_joint.py's


@pytest.fixture(scope="module", autouse=True)
def _device(lib_gpu):
    return lib_gpu


def _jd(shape, precision="fp64"):
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd.joint import joint_decoder
    L, M, n, z = SHAPES[shape]
    return joint_decoder(L, M, n, sp.LDPCParams("802.16", "5/6", z), T, precision=precision)


def _Pl(jd):
    return 4.0 / jd.L * np.ones(jd.L)


def _pack(jd, bits):
    w = 1 << np.arange(jd.logm - 1, -1, -1)
    return (bits.reshape(len(bits), jd.L, jd.logm).astype(np.int64) * w).sum(axis=2).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _reference(shape, seeds, sigma, mode):
    """jd.run on the device-drawn reps fetched back: computed once per case, never changed."""
    from sparc_ldpc_amd.joint import draw_reps_device
    jd = _jd(shape)
    idx, noise = draw_reps_device(jd, list(seeds), sigma)
    r = jd.run(idx, noise, _Pl(jd), mode)
    for v in r.values():
        v.setflags(write=False)
    return r


@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_device_draws_against_numpy(shape):
    from sparc_ldpc_amd.joint import draw_reps_device
    jd = _jd(shape)
    L, K, N, B = jd.L, jd.code.K, jd.code.N, len(SEEDS)
    U = jd.total_bits - N
    assert (K, N, U) == {"A": (160, 192, 64), "B": (480, 576, 192), "C": (160, 192, 0)}[shape]
    idx, noise = draw_reps_device(jd, SEEDS, 0.9)
    bits, _ = jd.code.joint_fetch(noise=False)
    assert jd.last_draw_ms > 0
    ref_idx, ref_noise = jd.draw([np.random.RandomState(s) for s in SEEDS], B, 0.9)
    assert idx.dtype == np.int32 and idx.shape == (B, L)
    np.testing.assert_array_equal(idx, ref_idx)
    assert noise.shape == ref_noise.shape == (B, jd.n)
    zero = ref_noise == 0
    ratio = np.abs(noise - ref_noise)[~zero] / np.abs(ref_noise[~zero])
    differ = int((noise != ref_noise).sum())
    print(f"{shape}: draw + encode {jd.last_draw_ms:.3f} ms, {differ} of {noise.size} noise values differ, "
          f"largest ratio {ratio.max() * 2.0 ** 52:.3f} * 2**-52")
    assert np.all(np.isfinite(noise))
    assert np.all(noise[zero] == 0)
    assert ratio.max() <= BAR
    # the raw message bits: the host's unprotected bits, then the codeword of the host's protected bits
    prot = np.empty((B, K), dtype=np.int64)
    unprot = np.empty((B, U), dtype=np.int64)
    for i, s in enumerate(SEEDS):
        rs = np.random.RandomState(s)
        prot[i] = rs.randint(0, 2, K)
        unprot[i] = rs.randint(0, 2, U)
    assert bits.dtype == np.uint8 and bits.shape == (B, U + N)
    np.testing.assert_array_equal(bits[:, U:], jd.code.encode_batch(prot))
    np.testing.assert_array_equal(bits[:, :U], unprot)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("shape", ["A", "C"])
def test_bit_packing_and_staging(shape, precision):
    """sa_encode_bits on the device buffers stages, bit for bit, what sa_encode
    stages from the same reps fetched back; its indices are the packed bits."""
    jd = _jd(shape, precision)
    op, B = jd.op, len(SEEDS)
    op.reserve(B, T)
    op.stage_power(B, _Pl(jd))
    d_bits, d_noise, _ = jd.draw_device(SEEDS, 0.9)
    idx = op.encode_bits(B, d_bits, d_noise)
    y_dev = op.fetch_y(B)
    bits, noise = jd.code.joint_fetch()
    idx_h = _pack(jd, bits)
    assert idx.dtype == np.int32
    np.testing.assert_array_equal(idx, idx_h)
    assert op.encode_bits(B, d_bits, d_noise, fetch_idx=False) is None
    op.encode(idx_h, noise)
    y_host = op.fetch_y(B)
    assert np.all(np.isfinite(y_dev)) and np.any(y_dev != 0)
    assert y_dev.tobytes() == y_host.tobytes()
    # the noise takes part: without it y differs
    op.encode_bits(B, d_bits, None)
    assert np.any(op.fetch_y(B) != y_dev)


@pytest.mark.parametrize("shape,mode", [("A", "originalHard"), ("A", "soft"), ("A", "hard"), ("A", "threshold"),
                                        ("B", "soft")])
def test_decode_on_device_draws(shape, mode):
    """mc_joint(draws="device") in batches of 16, 7 and 64 equals jd.run on the
    arrays of draw_reps_device, key by key.  sigma = 0.93 (A:
    tests/test_gpu_joint.py's; the first AMP leaves errors there, asserted)."""
    from sparc_ldpc_amd.joint import mc_joint
    jd = _jd(shape)
    sigma = SIGMA[shape]
    ref = _reference(shape, tuple(SEEDS37), sigma, mode)
    assert ref["amp"].shape[0] == len(SEEDS37)
    assert np.count_nonzero(ref["amp"][:, 0]) > 0, "all-zero counts compare nothing"
    for b in (16, 7, 64):
        r = mc_joint(jd, _Pl(jd), sigma, SEEDS37, mode, batch=b, draws="device")
        assert sorted(r) == sorted(ref)
        for k in ref:
            np.testing.assert_array_equal(r[k], ref[k], err_msg=f"{shape} {mode} batch {b}: {k}")


def test_pipeline_on_device_draws():
    from sparc_ldpc_amd.joint import mc_joint
    jd = _jd("A")
    seeds = range(300, 371)
    one = mc_joint(jd, _Pl(jd), 0.93, seeds, "soft", batch=71, draws="device", pipeline=False)
    two = mc_joint(jd, _Pl(jd), 0.93, seeds, "soft", batch=71, draws="device", pipeline=True)
    assert one["amp"].shape[0] == 71 and np.count_nonzero(one["amp"][:, 0]) > 0
    assert sorted(one) == sorted(two)
    for k in one:
        np.testing.assert_array_equal(two[k], one[k], err_msg=k)


def test_rejections():
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import _lib, ldpc
    from sparc_ldpc_amd.joint import draw_reps_device, mc_joint
    jd = _jd("A")
    Pl = _Pl(jd)
    with pytest.raises(ValueError, match="draws"):
        mc_joint(jd, Pl, 0.93, [1, 2], "soft", draws="gpu")
    with pytest.raises(ValueError, match="unit_cancel"):
        mc_joint(jd, Pl, 0.93, [1, 2], "threshold", unit_cancel=True, draws="device")
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError, match="Seed"):
            draw_reps_device(jd, [3, bad], 0.9)
        with pytest.raises(ValueError, match="Seed"):
            mc_joint(jd, Pl, 0.93, [3, bad], "soft", draws="device")
    # a K that is not the code's: LB_ERR_ARG, and the next valid draw is right
    code = jd.code
    code._set_encoder()
    lib = ldpc.load_bp_library()
    seeds = np.array(SEEDS, dtype=np.uint32)
    sp32 = seeds.ctypes.data_as(ct.POINTER(ct.c_uint32))
    U = jd.total_bits - code.N
    d_bits, d_noise = ct.c_void_p(), ct.c_void_p()
    for K, Ux, n, sigma in ((code.K - 1, U, jd.n, 0.9), (code.K, -1, jd.n, 0.9), (code.K, U, 0, 0.9),
                            (code.K, U, jd.n, float("inf")), (code.K, U, jd.n, float("nan"))):
        rc = lib.lb_joint_draw(code._context(), len(seeds), sp32, K, Ux, n, sigma, ct.byref(d_bits),
                               ct.byref(d_noise), None)
        assert rc == -1, (K, Ux, n, sigma)  # LB_ERR_ARG
        assert d_bits.value is None and d_noise.value is None
    idx, _ = draw_reps_device(jd, SEEDS, 0.9)
    ref_idx, _ = jd.draw([np.random.RandomState(s) for s in SEEDS], len(SEEDS), 0.9)
    np.testing.assert_array_equal(idx, ref_idx)
    # a code without its encoder set: LB_ERR_ARG
    bare = sp.code("802.16", "5/6", 8)
    rc = lib.lb_joint_draw(bare._context(), len(seeds), sp32, bare.K, U, jd.n, 0.9, ct.byref(d_bits),
                           ct.byref(d_noise), None)
    assert rc == -1 and b"lb_mc_set_code" in lib.lb_last_error()
    # M = 12 carries no whole bits: SA_ERR_UNSUPPORTED; no bits, no batch: SA_ERR_ARG
    db, dn, _ = jd.draw_device(SEEDS, 0.9)
    op12 = sp.SparcOperator(64, 12, 256, sp.make_ordering(64, 12, 256))
    op12.reserve(len(SEEDS), T)
    op12.stage_power(len(SEEDS), Pl)
    with pytest.raises(sp.SparcAmpError) as e:
        op12.encode_bits(len(SEEDS), db, dn)
    assert e.value.code == _lib.SA_ERR_UNSUPPORTED
    jd.op.reserve(len(SEEDS), T)
    jd.op.stage_power(len(SEEDS), Pl)
    with pytest.raises(sp.SparcAmpArgumentError):
        jd.op.encode_bits(len(SEEDS), None, dn)
    with pytest.raises(sp.SparcAmpArgumentError):
        jd.op.encode_bits(0, db, dn)
