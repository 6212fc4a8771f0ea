"""CPU: the argument checks of the device-draw entry points — the seed range
(NumPy's own ValueError, no masking) and the ``draws=`` option — are made
before any library call, so they need neither a device nor a context."""
import numpy as np
import pytest

BAD_SEEDS = [-1, 2 ** 32]
MSG = r"Seed must be between 0 and 2\*\*32 - 1"


class _NoDevice:
    """Stands in for an operator / a code: any use is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the check must come before any use of the object (.{name})")


def test_seed_array_keeps_numpys_range():
    from sparc_ldpc_amd.operators import seed_array
    out = seed_array([0, 1, 2 ** 31, 2 ** 32 - 1])
    assert out.dtype == np.uint32 and out.tolist() == [0, 1, 2 ** 31, 2 ** 32 - 1]
    assert seed_array(np.arange(3)).tolist() == [0, 1, 2]
    for bad in BAD_SEEDS:
        with pytest.raises(ValueError, match=MSG):
            seed_array([5, bad])
        with pytest.raises(ValueError):  # NumPy's own answer to the same seed
            np.random.RandomState(bad)


@pytest.mark.parametrize("bad", BAD_SEEDS)
def test_sparc_entry_points_refuse_seeds_outside_the_range(bad):
    import sparc_ldpc_amd as sp
    op = _NoDevice()
    with pytest.raises(ValueError, match=MSG):
        sp.SparcOperator.mc_draw(op, [1, bad], 0.5)
    with pytest.raises(ValueError, match=MSG):
        sp.mc_stream_seeds(op, np.ones(4), 8, [1, bad], 0.5)
    with pytest.raises(ValueError, match=MSG):
        sp.mc_decode(op, np.ones(4), 0.5, 8, [1, bad], draws="device")


@pytest.mark.parametrize("bad", BAD_SEEDS)
def test_ldpc_entry_points_refuse_seeds_outside_the_range(bad):
    from sparc_ldpc_amd import ldpc, ldpc_mc
    code = ldpc.code("802.16", "1/2", 24)  # host-side construction only
    with pytest.raises(ValueError, match=MSG):
        code.mc_blocks_seeds([1, bad], 0.8)
    with pytest.raises(ValueError, match=MSG):
        ldpc_mc.draw_blocks_device(code, [1, bad])
    with pytest.raises(ValueError, match=MSG):
        ldpc_mc.mc_ldpc(code, 0.8, [1, bad], draws="device")
    assert code._ctx is None  # no context was made


@pytest.mark.parametrize("draws", ["gpu", "Device", None, 1])
def test_draws_argument_is_checked(draws):
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc_awgn, ldpc_bsc, ldpc_mc
    nothing = _NoDevice()
    with pytest.raises(ValueError, match="draws must be"):
        sp.mc_decode(nothing, np.ones(4), 0.5, 8, [1, 2], draws=draws)
    with pytest.raises(ValueError, match="draws must be"):
        ldpc_mc.mc_ldpc(nothing, 0.8, [1, 2], draws=draws)
    with pytest.raises(ValueError, match="draws must be"):
        ldpc_mc._mc_point(nothing, 0.8, "awgn", 1, 1, 0, 4, draws=draws)
    with pytest.raises(ValueError, match="draws must be"):
        sp.sim_ldpc_mc(sp.LDPCParams("802.16", "1/2", 24), 0.8, draws=draws)
    with pytest.raises(ValueError, match="draws must be"):
        ldpc_awgn.sim("802.16", "1/2", 24, draws=draws)
    with pytest.raises(ValueError, match="draws must be"):
        ldpc_bsc.sim("802.16", "1/2", 24, draws=draws)


def test_host_draws_stay_the_default():
    import inspect
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc_awgn, ldpc_bsc, ldpc_mc
    for fn in (sp.mc_decode, ldpc_mc.mc_ldpc, ldpc_mc._mc_point, sp.sim_ldpc_mc, ldpc_awgn.sim, ldpc_bsc.sim):
        assert inspect.signature(fn).parameters["draws"].default == "host", fn.__name__


def test_draw_reps_still_masks_its_seeds():
    """The existing host entry point keeps its behaviour (seeds taken mod 2**32)."""
    import sparc_ldpc_amd as sp
    a = sp.draw_reps([2 ** 32 + 7], 4, 8, 6, 0.5)
    b = sp.draw_reps([7], 4, 8, 6, 0.5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
