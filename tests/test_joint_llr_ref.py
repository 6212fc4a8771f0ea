"""CPU: the NumPy statement of the two-sided LLR (tests/joint_llr_ref.py)
against oracle/glue_oracle.py's one-sided LLR, on hand vectors, and the reason
the two-sided form exists, pinned on a binary32-held β."""
import numpy as np
import pytest

import joint_llr_ref as jr
from oracle import glue_oracle as go


@pytest.mark.parametrize("prec", jr.PRECS)
@pytest.mark.parametrize("geom", jr.GEOMS, ids=jr.GEOM_IDS)
def test_statement_against_the_oracle(geom, prec):
    """|two − one| <= 2 |p0 + p1 − 1| / min(p0, p1) + 64 ε (|log p0| + |log p1|):
    the forms differ by log((1 − p1) / p0), and 1 − p1 = p0 − (p0 + p1 − 1)."""
    L, M, n, B, _ = geom
    Pl = jr.power(L)
    beta = jr.held(jr.draw(M, B, L, n, jr.LLR_SCALE[M]), prec)
    one, p = go.llr(beta, n, Pl, L, M, 0, L)
    two, p0, p1 = jr.two_sided_llr(beta, n, Pl, L, M, 0, L, prec)
    assert np.array_equal(p, p1)  # the reference's ordered sum on both sides
    assert p0.min() > 0 and p1.min() > 0
    bound = 2 * np.abs(p0 + p1 - 1) / np.minimum(p0, p1) + jr.log_bound(p0, p1)
    err = np.abs(np.asarray(two - one, dtype=np.float64))
    print(f"M={M} {prec}: max |two - one| / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("clip,mag", [(None, jr.F64_MAX), (0.0, jr.F64_MAX), (np.inf, jr.F64_MAX), (20.0, 20.0)])
@pytest.mark.parametrize("prec", jr.PRECS)
@pytest.mark.parametrize("geom", jr.GEOMS, ids=jr.GEOM_IDS)
def test_hand_vectors(geom, prec, clip, mag):
    L, M, n, B, _ = geom
    Pl = jr.power(L)
    beta, sign = jr.hand_vectors(B, L, M, n, Pl)
    got, _, _ = jr.two_sided_llr(jr.held(beta, prec), n, Pl, L, M, 0, L, prec, clip)
    assert not np.isnan(got).any()
    assert np.array_equal(np.asarray(got, dtype=np.float64), sign * mag)
    # all three kinds are there, and the reference form differs on the empty sections: +max
    assert {-1.0, 0.0, 1.0} <= set(np.unique(sign).tolist())
    one, _ = go.llr(jr.held(beta, prec), n, Pl, L, M, 0, L)
    empty = np.repeat((np.arange(B)[:, None] + np.arange(L)[None, :]) % 3 == 1, int(np.log2(M)), axis=1)
    assert np.all(np.asarray(one, dtype=np.float64)[empty] == jr.F64_MAX) and np.all(sign[empty] == 0)


@pytest.mark.parametrize("geom", [jr.GEOMS[0], jr.GEOMS[3]], ids=[jr.GEOM_IDS[0], jr.GEOM_IDS[3]])
def test_one_sided_form_erases_confident_bits_of_a_binary32_beta(geom):
    """β at scale 30 held in binary32: the oracle's one-sided LLR has exact
    zeros (p rounded above 1: NaN -> 0) on bits whose two-sided LLR is beyond
    16, and the two-sided LLR of the binary32 array stays within 1e-6 of the
    binary64 array's."""
    L, M, n, B, _ = geom
    Pl = jr.power(L)
    beta = jr.draw(M, B, L, n, jr.WIDE_SCALE)
    b32 = jr.held(beta, "fp32")
    one, _ = go.llr(b32, n, Pl, L, M, 0, L)
    two32, _, _ = jr.two_sided_llr(b32, n, Pl, L, M, 0, L, "fp32")
    two64, _, _ = jr.two_sided_llr(beta, n, Pl, L, M, 0, L, "fp64")
    one, two32, two64 = (np.asarray(v, dtype=np.float64) for v in (one, two32, two64))
    erased = (one == 0.0) & (np.abs(two32) > 16)
    print(f"M={M}: {int(erased.sum())} of {one.size} bits erased by the one-sided form, max |two| {np.abs(two32).max():.1f}")
    assert erased.any()
    fin = (np.abs(two32) < jr.F64_MAX) & (np.abs(two64) < jr.F64_MAX)
    assert fin.any() and np.abs(two32 - two64)[fin].max() <= 1e-6


def test_unknown_options_are_refused_before_any_device_work():
    """An unknown LLR form, a negative clip, an unknown decoder type and quant
    without layered_minsum: ValueError, before the operator or the code is touched."""
    from sparc_ldpc_amd import joint
    for bad in (dict(llr="both"), dict(llr_clip=-2.0), dict(llr_clip=float("nan")), dict(bp_dectype="layered"),
                dict(bp_dectype="sumprod2", bp_quant=True)):
        with pytest.raises(ValueError):
            joint.JointDecoder(64, 16, 256, None, 30, **bad)  # (no code object: it is never reached)
        with pytest.raises(ValueError):
            joint.joint_decoder(64, 16, 256, None, 30, **bad)
    with pytest.raises(TypeError):
        joint.joint_options(bp_algo="minsum")
    o = joint.joint_options(llr="two_sided", llr_clip=25, bp_dectype="layered_minsum", bp_quant=True)
    assert o["llr_clip"] == 25.0 and o["bp_quant"] == (2, 6, 8)
    assert joint.joint_options(llr_clip=0) == joint.joint_options(llr_clip=float("inf")) == joint.joint_options()
