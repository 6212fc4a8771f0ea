"""CPU: the LDPC-only Monte-Carlo's host side — the native seeded draws against
the NumPy definition of a block, seed validation, lb_mc_set_code's argument
checks, and the pure host logic of the AWGN / BSC sweeps (ldpc_awgn.sim,
ldpc_bsc.sim) against block-by-block restatements of the reference loops."""
import ctypes as ct

import numpy as np
import pytest

SEEDS = [0, 1, 12345, 2 ** 32 - 1]


@pytest.mark.parametrize("K,N", [(288, 576), (0, 72), (3840, 4608)])
@pytest.mark.parametrize("channel", ["awgn", "bsc"])
@pytest.mark.parametrize("threads", [1, 3])
def test_draw_blocks_equals_numpy_definition(K, N, channel, threads):
    from sparc_ldpc_amd import ldpc_mc
    u0, w0 = ldpc_mc._draw_blocks(SEEDS, K, N, channel)
    u1, w1 = ldpc_mc.draw_blocks(SEEDS, K, N, channel, threads=threads)
    if K == 0:
        assert u0 is None and u1 is None
    else:
        assert u1.dtype == np.uint8 and u1.shape == (len(SEEDS), K)
        assert np.array_equal(u0, u1)
        assert set(np.unique(u1)) == {0, 1}
    assert w1.shape == (len(SEEDS), N)
    assert w0.tobytes() == w1.tobytes()  # bit for bit


def test_draw_blocks_definition_is_the_seed_contract():
    """_draw_blocks itself: randint(0, 2, K) then randn(N) / random_sample(N) of RandomState(s)."""
    from sparc_ldpc_amd import ldpc_mc
    u, w = ldpc_mc._draw_blocks([7], 5, 9, "awgn")
    rs = np.random.RandomState(7)
    assert np.array_equal(u[0], rs.randint(0, 2, 5)) and np.array_equal(w[0], rs.randn(9))
    u, w = ldpc_mc._draw_blocks([7], 0, 9, "bsc")
    assert u is None and np.array_equal(w[0], np.random.RandomState(7).random_sample(9))


@pytest.mark.parametrize("bad", [-1, 2 ** 32])
def test_seeds_outside_range_raise(bad):
    from sparc_ldpc_amd import ldpc_mc
    with pytest.raises(ValueError):
        ldpc_mc.draw_blocks([3, bad], 4, 8)
    with pytest.raises(ValueError):
        ldpc_mc._draw_blocks([3, bad], 4, 8)


def test_mc_set_code_argument_checks():
    from sparc_ldpc_amd import ldpc
    lib = ldpc.load_bp_library()
    c = ldpc.code("802.16", "1/2", 3)
    good = np.ascontiguousarray(c.proto, dtype=np.intc)
    Mp, Np = good.shape
    IP = ct.POINTER(ct.c_int)
    # a valid base matrix passes the host checks: only the null context is left to refuse
    assert lib.lb_mc_set_code(None, good.ctypes.data_as(IP), Mp, Np, 3) == -1
    assert b"null context" in lib.lb_last_error()
    # column Kp with three surviving offsets: refused before the context is looked at
    bad = good.copy()
    rows = np.nonzero(bad[:, Np - Mp] != -1)[0]
    assert len(rows) == 3
    bad[rows, Np - Mp] = [0, 1, 2]  # three distinct offsets survive
    with pytest.raises(NameError):
        ldpc.encode_batch(bad, 3, np.zeros((1, c.K), dtype=int))
    assert lib.lb_mc_set_code(None, bad.ctypes.data_as(IP), Mp, Np, 3) == -1
    assert b"single offset" in lib.lb_last_error()
    assert lib.lb_mc_set_code(None, None, 0, 0, 0) == -1  # no encoder, null context
    assert b"null context" in lib.lb_last_error()
    if lib.lb_device_count() > 0:
        assert lib.lb_mc_set_code(c._context(), bad.ctypes.data_as(IP), Mp, Np, 3) == -1
        assert b"single offset" in lib.lb_last_error()


def test_sim_param_grids():
    from sparc_ldpc_amd import ldpc, ldpc_awgn, ldpc_bsc
    for mod, z0 in ((ldpc_awgn, 3), (ldpc_bsc, 100)):
        assert len(mod.sim_param) == 36 and len(set(mod.sim_param)) == 36
        for std, rate, z, ptype in mod.sim_param:
            proto = ldpc.assign_proto(std, rate, z, ptype)
            assert proto.shape[1] == 24
        assert mod.sim_param[0] == ("802.16", "1/2", z0, "A")
        assert [p[2] for p in mod.sim_param[:24:6]] == [z0, 27, 54, 81]
        assert mod.sim_param[24] == ("802.11n", "1/2", 27, "A") and mod.sim_param[35] == ("802.11n", "5/6", 81, "A")


def _fake_mc_ldpc(code, a, seeds, channel="awgn", batch=1024, dectype="sumprod2", drawn=None, **kw):
    """Deterministic stand-in for ldpc_mc.mc_ldpc: a block fails more often at a
    larger sigma / p, as a function of its seed alone."""
    s = np.asarray(list(seeds), dtype=np.int64)
    scale = 1.0 if channel == "awgn" else 8.0
    fails = ((s * 2654435761) % 1000) / 1000.0 < min(0.9, scale * a * a)
    be = np.where(fails, (s * 7) % 11 + 1, 0).astype(np.int64)
    return be, (s % 5 + 10).astype(np.int64)


def _awgn_reference_loop(standard, rate, z, K, N_MEASUREMENTS, C_AWGN_OFFSET, P_STEP, MIN_ERRORS, MAX_BLOCKS, seed0):
    """ldpc_awgn.py:60-123 written out block by block over the seeded blocks."""
    R = {"1/2": .5, "2/3": 0.6667, "3/4": 0.75, "5/6": 0.83333}[rate]
    SNR = 10.0 * np.log10(np.power(2, R) - 1.0) + C_AWGN_OFFSET
    res = []
    for datapoint in range(N_MEASUREMENTS):
        nbiterrors = nblockerrors = nblocks = nit_total = 0
        sigma2 = 1 / np.power(10, SNR / 10.0)
        s = seed0 + datapoint * 10_000_000
        while nblockerrors < MIN_ERRORS:
            be, it = _fake_mc_ldpc(None, float(np.sqrt(sigma2)), [s])
            s += 1
            nbiterrors += int(be[0])
            if be[0]:
                nblockerrors += 1
            nblocks += 1
            nit_total += int(it[0])
            if nblocks >= MAX_BLOCKS:
                break
        res.append((standard, rate, z, SNR, nblocks, nblockerrors, nblocks * K, nbiterrors, nit_total))
        SNR += np.sqrt(P_STEP / nblocks)
    return res


@pytest.mark.parametrize("min_errors,max_blocks,batch", [(4, 60, 8), (50, 13, 5), (2, 1000, 1)])
def test_ldpc_awgn_sim_equals_reference_loop(monkeypatch, tmp_path, min_errors, max_blocks, batch):
    from sparc_ldpc_amd import ldpc, ldpc_awgn, ldpc_mc
    monkeypatch.setattr(ldpc_mc, "mc_ldpc", _fake_mc_ldpc)
    out = tmp_path / "results.txt"
    got = ldpc_awgn.sim("802.16", "2/3", 3, "B", N_MEASUREMENTS=6, C_AWGN_OFFSET=1.0, P_STEP=100.0,
                        MIN_ERRORS=min_errors, MAX_BLOCKS=max_blocks, seed0=500, batch=batch, results_file=str(out))
    K = ldpc.code("802.16", "2/3", 3, "B").K
    want = _awgn_reference_loop("802.16", "2/3", 3, K, 6, 1.0, 100.0, min_errors, max_blocks, 500)
    assert got == want
    assert len({t[3] for t in got}) == 6  # the SNR moved at every point
    assert out.read_text() == "".join(str(t) + "\n" for t in want)
    with pytest.raises(NameError):
        ldpc_awgn.sim("802.16", "7/8", 3)


def test_ldpc_bsc_sim_equals_reference_loop(monkeypatch):
    from sparc_ldpc_amd import ldpc, ldpc_bsc, ldpc_mc
    monkeypatch.setattr(ldpc_mc, "mc_ldpc", _fake_mc_ldpc)
    res, parray = ldpc_bsc.sim("802.16", "3/4", 3, "A", repeats=40, seed0=900)
    assert np.array_equal(parray, np.linspace(0.0415, 0.001, 10))
    N = ldpc.code("802.16", "3/4", 3, "A").N
    want = []
    for i, q in enumerate(parray):  # ldpc_bsc.py:93-111
        errors = []
        for k in range(40):
            be, _ = _fake_mc_ldpc(None, float(q), [900 + i * 10_000_000 + k], channel="bsc")
            errors.append(int(be[0]) / N)
        want.append(np.sum(errors) / 40)
    assert res == want and any(r > 0 for r in res)
    with pytest.raises(NameError):
        ldpc_bsc.sim("802.16", "0.45", 3)


def test_ber_point_reports_integer_iterations_total():
    import sparc_ldpc_amd as sp
    r = sp.ber_point(lambda seeds: _fake_mc_ldpc(None, 0.8, seeds), 72, 3, 40, 4, seed_base=100)
    be, it = _fake_mc_ldpc(None, 0.8, range(100, 100 + r["blocks"]))
    assert isinstance(r["iters_total"], int) and r["iters_total"] == int(it.sum())
    assert r["bit_errors"] == int(be.sum()) and r["mean_iters"] == r["iters_total"] / r["blocks"]
