"""CPU: the host side of the streamed LDPC Monte-Carlo point
(ldpc_mc stream=True, harness.consume_in_seed_order, lb_mc_stream_seeds'
place in the export table).  No device is needed."""
import numpy as np
import pytest


def _ber_point_over(be, it, total_bits, min_errors, max_blocks, batch):
    """harness.ber_point fed from per-block arrays in rounds of ``batch``"""
    from sparc_ldpc_amd.harness import ber_point
    pos = [0]

    def decode_round(seeds):
        assert list(seeds) == list(range(pos[0], pos[0] + batch))
        b0 = pos[0]
        pos[0] += batch
        pad = lambda v: np.concatenate([v[b0:b0 + batch], np.zeros(max(0, b0 + batch - len(v)), dtype=np.int64)])
        return pad(be), pad(it)

    return ber_point(decode_round, total_bits, min_errors, max_blocks, batch)


def _arrays(n, fail_at, seed):
    rs = np.random.RandomState(seed)
    be = np.zeros(n, dtype=np.int64)
    be[list(fail_at)] = rs.randint(1, 50, len(fail_at))
    it = rs.randint(0, 201, n).astype(np.int64)
    return be, it


# (blocks, failing blocks, min_errors, max_blocks): what ends the point
CASES = {
    "met_mid_round": (200, [3, 9, 30, 31, 70, 100], 4, 200),          # stops at block 31: inside a round of 7 and of 64
    "met_on_last_block_of_a_round": (200, [5, 20, 63, 150], 3, 200),  # block 63 ends a round of 64; 62 = 7 * 9 - 1 below
    "met_on_last_block_of_a_round_of_7": (200, [5, 20, 62, 150], 3, 200),
    "never_met": (128, [1, 100], 5, 128),                             # max_blocks ends it, a multiple of 64
    "max_blocks_not_a_multiple": (137, [0, 50, 136], 10, 137),        # 137 = 2 * 64 + 9 = 19 * 7 + 4
    "met_on_the_very_last_block": (137, [0, 50, 136], 3, 137),
    "first_block": (50, [0], 1, 50),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("batch", [7, 64])
def test_consume_in_seed_order_equals_ber_point(name, batch):
    from sparc_ldpc_amd.harness import consume_in_seed_order
    n, fail_at, min_errors, max_blocks = CASES[name]
    be, it = _arrays(n, fail_at, 11)
    want = _ber_point_over(be, it, 648, min_errors, max_blocks, batch)
    got = consume_in_seed_order(be, it, 648, min_errors, max_blocks)
    assert got == want
    assert repr(got["BER"]) == repr(want["BER"]) and repr(got["mean_iters"]) == repr(want["mean_iters"])
    cum = np.cumsum(be > 0)
    nstar = int(np.argmax(cum >= min_errors)) + 1 if cum[-1] >= min_errors else max_blocks
    assert got["blocks"] == min(nstar, max_blocks)


def test_consume_in_seed_order_does_not_read_behind_the_stopping_block():
    from sparc_ldpc_amd.harness import consume_in_seed_order
    be, it = _arrays(100, [2, 10, 40], 7)
    full = consume_in_seed_order(be, it, 648, 2, 100)
    assert full["blocks"] == 11
    be[11:] = 999  # what a skipped block holds must not matter
    it[11:] = -1
    assert consume_in_seed_order(be, it, 648, 2, 100) == full


class _NoDevice:
    """a code that fails the test if anything reaches the library"""
    N, K, standard = 648, 324, "802.11n"

    def __getattr__(self, name):
        raise AssertionError(f"stream=True reached code.{name} before its arguments were checked")


@pytest.mark.parametrize("kw", [dict(draws="host", dectype="layered_sumprod2"),
                                dict(draws="device", dectype="sumprod2"),
                                dict(draws="device", dectype="layered_sumprod2", world=2)],
                         ids=["host_draws", "flooding", "two_ranks"])
def test_stream_rejects_what_it_cannot_run_before_any_library_call(kw, monkeypatch):
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc, ldpc_awgn, ldpc_bsc, ldpc_mc

    def no_code(*a, **k):
        raise AssertionError("stream=True built a code before its arguments were checked")

    monkeypatch.setattr(ldpc, "code", no_code)
    monkeypatch.setattr(ldpc, "load_bp_library", no_code)
    with pytest.raises(ValueError):
        ldpc_mc._mc_point(_NoDevice(), 0.8, "awgn", 5, 100, 0, 16, stream=True, **kw)
    with pytest.raises(ValueError):
        sp.sim_ldpc_mc(sp.LDPCParams("802.16", "5/6", 8), 0.56, MIN_ERRORS=5, MAX_BLOCKS=100, stream=True, **kw)
    if "world" in kw:
        return  # mc_ldpc and the two sweeps have no ranks
    with pytest.raises(ValueError):
        ldpc_mc.mc_ldpc(_NoDevice(), 0.8, range(4), stream=True, **kw)
    with pytest.raises(ValueError):
        ldpc_awgn.sim("802.16", "5/6", 8, N_MEASUREMENTS=1, stream=True, **kw)
    with pytest.raises(ValueError):
        ldpc_bsc.sim("802.16", "5/6", 8, repeats=4, stream=True, **kw)


def test_stream_keyword_defaults_to_off():
    import inspect

    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc_awgn, ldpc_bsc, ldpc_mc
    for fn in (ldpc_mc.mc_ldpc, ldpc_mc._mc_point, sp.sim_ldpc_mc, ldpc_awgn.sim, ldpc_bsc.sim):
        assert inspect.signature(fn).parameters["stream"].default is False, fn


def test_stream_entry_point_is_declared_exported_and_typed():
    """(test_bp_library_exports_every_header_symbol holds the whole table)"""
    import ctypes as ct
    import os

    from sparc_ldpc_amd import ldpc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ldpc_bp.h")) as fh:
        assert "int lb_mc_stream_seeds(" in fh.read()
    assert "lb_mc_stream_seeds" in ldpc.EXPORTS
    assert hasattr(ct.CDLL(ldpc.LIB_PATH), "lb_mc_stream_seeds")
    res, args = ldpc._SIG["lb_mc_stream_seeds"]
    assert res is ct.c_int and len(args) == 15
