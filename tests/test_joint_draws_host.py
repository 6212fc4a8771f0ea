"""CPU: the positions in NumPy's legacy stream that the device draw of a joint
SPARC + LDPC rep relies on (csrc/ldpc_mc.hip k_joint_draw).  For
RandomState(s): randint(0, 2, K), randint(0, 2, U) and randn(n) consume the
output words one after another, a randint(0, 2) value being its word & 1 (the
mask of the range is the range itself: nothing is rejected), and randn starts at
word K + U with no cached Gaussian."""
import numpy as np
import pytest

# (seed, K, U, n): U = 0 (no second randint); K + U > 624 (the second randint and
# the start of randn lie in the second output block); one below a block's end
CASES = [(7, 160, 0, 191), (2 ** 32 - 1, 480, 192, 384), (1003, 400, 223, 33)]


@pytest.mark.parametrize("seed,K,U,n", CASES)
def test_word_positions_of_a_joint_rep(seed, K, U, n):
    rs = np.random.RandomState(seed)
    prot = rs.randint(0, 2, K)
    unprot = rs.randint(0, 2, U)
    noise = rs.randn(n)

    ws = np.random.RandomState(seed)
    words = ws.randint(0, 2 ** 32, K + U, dtype=np.uint32)
    np.testing.assert_array_equal(words[:K] & 1, prot)
    np.testing.assert_array_equal(words[K:] & 1, unprot)
    np.testing.assert_array_equal(ws.randn(n), noise)  # from word K + U on, nothing cached


def test_library_declares_the_joint_draw_entries():
    """The hand-off between the two libraries: both sides are declared, exported and typed."""
    import ctypes as ct

    from sparc_ldpc_amd import _lib, ldpc
    bp = ct.CDLL(ldpc.LIB_PATH)
    for name, nargs in (("lb_joint_draw", 10), ("lb_joint_fetch", 4)):
        assert name in ldpc.EXPORTS and hasattr(bp, name)
        assert len(ldpc._SIG[name][1]) == nargs
    assert "sa_encode_bits" in _lib.EXPORTS and hasattr(ct.CDLL(_lib.LIB_PATH), "sa_encode_bits")
    assert len(_lib._SIG["sa_encode_bits"][1]) == 5


def test_draws_keyword_is_checked_before_any_device_call():
    from sparc_ldpc_amd import joint
    with pytest.raises(ValueError, match="draws"):
        joint.mc_joint(None, None, 0.9, [1], "soft", draws="gpu")
    with pytest.raises(ValueError, match="unit_cancel"):
        joint.mc_joint(None, None, 0.9, [1], "threshold", unit_cancel=True, draws="device")
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError, match="Seed"):
            joint.mc_joint(None, None, 0.9, [5, bad], "soft", draws="device")
