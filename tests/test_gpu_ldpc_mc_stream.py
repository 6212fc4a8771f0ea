"""GPU: one LDPC Monte-Carlo point streamed through refilled decoder slots
(lb_mc_stream_seeds: the persistent layered decode-and-count kernels k_bpls /
k_bpls32) against the batch path on the same seeds (lb_mc_run_seeds:
code.mc_blocks_seeds, _mc_point(stream=False)).  Everything is integers per
block: every comparison is exact.  The reference is never the stream itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYERED = ["layered_sumprod2", "layered_minsum", "layered_sumprod2_f32", "layered_minsum_f32"]
SEEDS = np.arange(100, 400)  # 300 blocks
# (chunk, slots): a partial last chunk; one workgroup that reuses its image 37 times in a row,
# after failed and clean words alike; a block a chunk; chunk = the blocks; chunk > the blocks
# (default slots); more slots than a chunk has blocks
SHAPES = [(64, 3), (37, 1), (1, 2), (300, 0), (1000, 0), (128, 500)]

# name -> (standard, rate, z, channel, a); a = None: found from the batch path (_sigma_from_batch)
CASES = {
    "11n-1/2-z27": ("802.11n", "1/2", 27, "awgn", 0.85),
    "16-5/6-z8": ("802.16", "5/6", 8, "awgn", 0.56),
    "16-5/6-z24-dcfix20": ("802.16", "5/6", 24, "awgn", None),
    # the degree classes 16 (checks of 14 and 15 edges) and 32 (22 edges: regular, but not the straight-line 20)
    "16-3/4-z24-dc16": ("802.16", "3/4", 24, "awgn", 0.62),
    "11n-5/6-z27-dc32": ("802.11n", "5/6", 27, "awgn", 0.54),
    "2_7_12_good-K0": ("2_7_12_good", "1/2", 16, "awgn", None),
    "bsc-p0.03": ("802.11n", "1/2", 27, "bsc", 0.03),
}

_codes, _ref, _sigma = {}, {}, {}
# noise levels to try, by rate, where the issue names none
LADDER = {"5/6": (0.50, 0.52, 0.54, 0.56, 0.58, 0.60, 0.62), "1/2": (0.80, 0.84, 0.88, 0.92, 0.96, 1.00, 1.04)}


def _code(std, rate, z):
    from sparc_ldpc_amd import ldpc
    if (std, rate, z) not in _codes:
        _codes[(std, rate, z)] = ldpc.code(std, rate, z)
    return _codes[(std, rate, z)]


def _sigma_from_batch(std, rate, z):
    """A case's noise level taken from the batch path: the first of its rate's
    fixed ladder at which the 300 blocks hold at least 20 clean and 20 failed
    ones under every layered decoder."""
    key = (std, rate, z)
    if key not in _sigma:
        code = _code(*key)
        for sigma in LADDER[rate]:
            mixed = True
            for dectype in LAYERED:
                be, _ = code.mc_blocks_seeds(SEEDS, sigma, "awgn", 64, dectype)
                mixed = mixed and min(int((be > 0).sum()), int((be == 0).sum())) >= 20
            if mixed:
                _sigma[key] = sigma
                break
        assert key in _sigma, "no noise level of the ladder leaves both clean and failed blocks"
    return _sigma[key]


def _sigma_z24():
    return _sigma_from_batch("802.16", "5/6", 24)


def _case(name):
    std, rate, z, channel, a = CASES[name]
    return _code(std, rate, z), channel, (_sigma_from_batch(std, rate, z) if a is None else a)


def _batch(name, dectype, max_iter=200):
    """the batch path's per-block result of a case, computed once"""
    key = (name, dectype, max_iter)
    if key not in _ref:
        code, channel, a = _case(name)
        be, it = code.mc_blocks_seeds(SEEDS, a, channel, 64, dectype, max_iter=max_iter)
        be.setflags(write=False)
        it.setflags(write=False)
        _ref[key] = (be, it)
    return _ref[key]


@pytest.mark.parametrize("dectype", LAYERED)
@pytest.mark.parametrize("name", sorted(CASES))
def test_stream_equals_batch_per_block(lib_gpu, name, dectype):
    code, channel, a = _case(name)
    be0, it0 = _batch(name, dectype)
    failed, clean = int((be0 > 0).sum()), int((be0 == 0).sum())
    print(f"{name} {dectype} a={a}: failed={failed} clean={clean} mean sweeps={it0.mean():.2f}")
    if channel == "awgn":
        assert failed and clean, "the case must hold both clean and failed blocks"
    if name == "16-5/6-z24-dcfix20":
        assert code.layer_info()["threads"] <= 768 and int(code.cdeg.min()) == int(code.cdeg.max()) == 20
    for chunk, slots in SHAPES:
        be, it, info = code.mc_stream_seeds(SEEDS, a, channel, chunk, dectype, slots=slots)
        assert be.dtype == np.int64 and it.dtype == np.int64
        np.testing.assert_array_equal(be, be0, err_msg=f"chunk {chunk} slots {slots}")
        np.testing.assert_array_equal(it, it0, err_msg=f"chunk {chunk} slots {slots}")
        nchunks = -(-len(SEEDS) // min(chunk, len(SEEDS)))
        assert info["used"] == info["decoded"] == len(SEEDS) and info["chunks"] == nchunks, (chunk, slots, info)
        assert 1 <= info["slots"] <= min(chunk, len(SEEDS))
        if slots > 0:
            assert info["slots"] == min(slots, chunk, len(SEEDS))


@pytest.mark.parametrize("dectype", LAYERED)
@pytest.mark.parametrize("max_iter", [0, 3])
def test_stream_equals_batch_at_small_max_iter(lib_gpu, dectype, max_iter):
    name = "16-5/6-z8"
    code, channel, a = _case(name)
    be0, it0 = _batch(name, dectype, max_iter)
    assert it0.max() == max_iter and (be0 > 0).any()
    for chunk, slots in [(64, 3), (37, 1), (300, 0)]:
        be, it, _ = code.mc_stream_seeds(SEEDS, a, channel, chunk, dectype, max_iter=max_iter, slots=slots)
        np.testing.assert_array_equal(be, be0, err_msg=f"chunk {chunk} slots {slots}")
        np.testing.assert_array_equal(it, it0, err_msg=f"chunk {chunk} slots {slots}")


@pytest.mark.parametrize("lds", ["1", "0"])
@pytest.mark.parametrize("rate", ["1/2", "5/6"])
def test_stream_with_messages_in_hbm(lib_gpu, monkeypatch, lds, rate):
    """r (1) / r and app (0) in slot-indexed HBM slices that every next word of
    the slot reuses; two slots for 300 words."""
    from sparc_ldpc_amd import ldpc
    sigma = _sigma_from_batch("802.16", rate, 24)
    monkeypatch.setenv("LDPC_BP_LAYERED_LDS", lds)
    code = ldpc.code("802.16", rate, 24)  # its own context: the layers are set under the switch
    for dectype in ("layered_sumprod2", "layered_sumprod2_f32", "layered_minsum", "layered_minsum_f32"):
        be0, it0 = code.mc_blocks_seeds(SEEDS, sigma, "awgn", 64, dectype)
        precision = "f32" if dectype.endswith("_f32") else "f64"
        assert code.layer_info(precision)["lds_messages"] == int(lds)
        print(f"802.16 {rate} z=24 LDS={lds} {dectype}: failed={int((be0 > 0).sum())} clean={int((be0 == 0).sum())}")
        assert (be0 > 0).any() and (be0 == 0).any()
        for chunk in (64, 300):
            be, it, info = code.mc_stream_seeds(SEEDS, sigma, "awgn", chunk, dectype, slots=2)
            assert info["slots"] == 2
            np.testing.assert_array_equal(be, be0, err_msg=f"{dectype} chunk {chunk}")
            np.testing.assert_array_equal(it, it0, err_msg=f"{dectype} chunk {chunk}")


RULE_SEEDS = np.arange(5000, 5600)  # 600 blocks


@pytest.mark.parametrize("dectype", ["layered_sumprod2", "layered_minsum_f32"])
def test_stop_rule(lib_gpu, dectype):
    code = _code("802.16", "5/6", 8)
    nblk = len(RULE_SEEDS)
    # a noise level with few failed blocks (two slots decode all 600 in turn, and a failed block
    # runs 200 sweeps): the first of a fixed ladder that leaves at least 8
    for sigma in (0.44, 0.46, 0.48, 0.50, 0.52, 0.54, 0.56):
        be0, it0 = code.mc_blocks_seeds(RULE_SEEDS, sigma, "awgn", 64, dectype)
        if int((be0 > 0).sum()) >= 8:
            break
    cum = np.cumsum(be0 > 0)
    E = int(cum[-1])
    print(f"{dectype} sigma={sigma}: E={E} of {nblk}, first failed block {int(np.argmax(cum >= 1))}")
    assert 8 <= E < nblk, E
    for min_errors in sorted({1, 2, E // 2, E, E + 1}):
        nstar = int(np.argmax(cum >= min_errors)) + 1 if min_errors <= E else nblk
        for chunk in sorted({max(1, nstar - 1), nstar, nstar + 1, 50}):
            for slots in (0, 2):
                be, it, info = code.mc_stream_seeds(RULE_SEEDS, sigma, "awgn", chunk, dectype,
                                                    min_errors=min_errors, slots=slots)
                tag = f"min_errors {min_errors} n* {nstar} chunk {chunk} slots {slots} {info}"
                assert info["used"] == nstar, tag
                np.testing.assert_array_equal(be[:nstar], be0[:nstar], err_msg=tag)
                np.testing.assert_array_equal(it[:nstar], it0[:nstar], err_msg=tag)
                skipped = it[nstar:] == -1
                assert np.all(be[nstar:][skipped] == 0), tag
                np.testing.assert_array_equal(be[nstar:][~skipped], be0[nstar:][~skipped], err_msg=tag)
                np.testing.assert_array_equal(it[nstar:][~skipped], it0[nstar:][~skipped], err_msg=tag)
                assert info["decoded"] == int((it != -1).sum()), tag
                # two chunks in flight: the host queues nothing behind the chunk after n*'s
                c = min(chunk, nblk)
                assert info["decoded"] <= (-(-nstar // c) + 1) * c, tag
                assert info["chunks"] <= -(-nstar // c) + 1, tag


@pytest.mark.parametrize("rule", [(5, 400), (1000, 137)], ids=["met", "max_blocks"])
def test_python_layers_equal_the_batch_path(lib_gpu, rule):
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc_awgn, ldpc_bsc, ldpc_mc
    min_errors, max_blocks = rule
    code = _code("802.16", "5/6", 8)
    for dectype in ("layered_sumprod2", "layered_sumprod2_f32"):
        kw = dict(dectype=dectype, draws="device")
        t0, t1 = {}, {}
        want = ldpc_mc._mc_point(code, 0.56, "awgn", min_errors, max_blocks, 700, 64, timings=t0, **kw)
        got = ldpc_mc._mc_point(code, 0.56, "awgn", min_errors, max_blocks, 700, 64, timings=t1, stream=True, **kw)
        assert got == want and repr(got["BER"]) == repr(want["BER"])
        assert t1["device_ms"] > 0 and t1["stream"]["used"] == want["blocks"]
        if min_errors == 5:
            assert want["block_errors"] == 5 and want["blocks"] < max_blocks
        else:
            assert want["blocks"] == max_blocks
        lp = sp.LDPCParams("802.16", "5/6", 8)
        want = sp.sim_ldpc_mc(lp, 0.56, MIN_ERRORS=min_errors, MAX_BLOCKS=max_blocks, seed0=9, batch=50, **kw)
        got = sp.sim_ldpc_mc(lp, 0.56, MIN_ERRORS=min_errors, MAX_BLOCKS=max_blocks, seed0=9, batch=50, stream=True,
                             **kw)
        assert got == want and repr(got["ber"]) == repr(want["ber"])
    kw = dict(N_MEASUREMENTS=2, MIN_ERRORS=min_errors, MAX_BLOCKS=max_blocks, seed0=3, batch=64, draws="device",
              dectype="layered_minsum_f32")
    want = ldpc_awgn.sim("802.16", "5/6", 24, **kw)
    assert ldpc_awgn.sim("802.16", "5/6", 24, stream=True, **kw) == want
    assert [r[4] for r in want] == [max_blocks] * 2 or min_errors == 5
    kw = dict(repeats=37, seed0=1, draws="device", dectype="layered_sumprod2")
    res0, p0 = ldpc_bsc.sim("802.16", "5/6", 8, **kw)
    res1, p1 = ldpc_bsc.sim("802.16", "5/6", 8, stream=True, **kw)
    assert res0 == res1 and np.array_equal(p0, p1)
    be0, it0 = ldpc_mc.mc_ldpc(code, 0.56, range(40), batch=16, dectype="layered_minsum", draws="device")
    be1, it1 = ldpc_mc.mc_ldpc(code, 0.56, range(40), batch=16, dectype="layered_minsum", draws="device", stream=True)
    np.testing.assert_array_equal(be1, be0)
    np.testing.assert_array_equal(it1, it0)


def test_stream_leaves_the_context_as_it_was(lib_gpu):
    from sparc_ldpc_amd import ldpc
    code = ldpc.code("802.16", "5/6", 24)
    sigma = _sigma_z24()
    rs = np.random.RandomState(3)
    CH = 2.0 * (1.0 + sigma * rs.randn(24, code.N)) / sigma ** 2

    def snapshot():
        out = []
        for dectype in ("sumprod2", "minsum", "layered_sumprod2", "layered_minsum_f32"):
            app, it = code.decode_batch(CH, dectype)
            out += [app.tobytes(), it.tobytes()]
            be, it = code.mc_blocks_seeds(SEEDS[:80], sigma, "awgn", 32, dectype)
            out += [be.tobytes(), it.tobytes()]
        return out

    before = snapshot()
    for dectype in ("layered_sumprod2", "layered_minsum_f32"):
        code.mc_stream_seeds(SEEDS, sigma, "awgn", 64, dectype, slots=3)
        code.mc_stream_seeds(SEEDS, sigma, "awgn", 50, dectype, min_errors=2)
    assert snapshot() == before
    for dectype in ("sumprod2", "minsum", "sumprod"):
        with pytest.raises(ldpc.LdpcBpError) as e:
            code.mc_stream_seeds(SEEDS, sigma, "awgn", 64, dectype)
        assert e.value.code == -5
    with pytest.raises(AssertionError):  # LB_ERR_ARG
        code.mc_stream_seeds(SEEDS, sigma, "awgn", 0, "layered_sumprod2")
    with pytest.raises(AssertionError):
        code.mc_stream_seeds(SEEDS, -1.0, "awgn", 64, "layered_sumprod2")
    with pytest.raises(AssertionError):
        code.mc_stream_seeds(SEEDS, sigma, "awgn", 64, "layered_sumprod2", max_iter=-1)
    assert snapshot() == before
    # no layers set: LB_ERR_ARG from the library itself
    bare = ldpc.code("802.16", "5/6", 24)
    bare._set_encoder()
    seeds = np.ascontiguousarray(SEEDS, dtype=np.uint32)
    import ctypes as ct
    errs, its, out = np.zeros(300, np.intc), np.zeros(300, np.intc), (ct.c_int64 * 4)()
    rc = ldpc.load_bp_library().lb_mc_stream_seeds(
        bare._context(), 300, seeds.ctypes.data_as(ct.POINTER(ct.c_uint32)), bare.K, sigma, 0, 64, 0, 0,
        ldpc.LB_LAYERED_SUMPROD2, 0.7, 200, errs.ctypes.data_as(ldpc._IP), its.ctypes.data_as(ldpc._IP), out)
    assert rc == -1 and b"layers" in ldpc.load_bp_library().lb_last_error()
    app, it = bare.decode_batch(CH, "sumprod2")
    assert [app.tobytes(), it.tobytes()] == before[:2]
