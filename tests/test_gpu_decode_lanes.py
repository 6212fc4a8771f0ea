"""Decode lanes: consecutive small-batch decodes of one context alternate
between two in-context lanes (a stream and everything a decode mutates) and
overlap on the chip when the caller pipelines them (the next step issued
while the previous one's decisions are uncollected: the protocol of every test
here, so the lanes alternate from the second step on, whatever the timing).
Every result is compared bit for bit (np.array_equal)
with a single-lane operator (plan NO_LANES) and with a fresh operator per
input.  Shapes of test_gpu_single_tail.py: (256, 256, 2048) runs k_sec4 +
k_row2, (64, 512, 581) k_sec + k_row2; T <= 6."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import amp_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [(256, 256, 2048), (64, 512, 581)]
PRECS = ["fp32", "fp64"]


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


_ORACLE, _ORDER, _YS, _REF = {}, {}, {}, {}


def ordering(sp, L, M, n):
    if (L, M, n) not in _ORDER:
        _ORDER[(L, M, n)] = sp.make_ordering(L, M, n)
    return _ORDER[(L, M, n)]


def power(L, P=2.0):
    return P / L * np.ones(L)


def inputs(L, M, n, count=6):
    """`count` different received words of a shape (1, n) each, built once."""
    key = (L, M, n, count)
    if key not in _YS:
        if (L, M, n) not in _ORACLE:
            _ORACLE[(L, M, n)] = orc.sparc_transforms(L, M, n)[0]
        Ab = _ORACLE[(L, M, n)]
        _YS[key] = [orc.rep_inputs(L, M, n, power(L), 0.6, Ab, 900 + i)[1].reshape(1, -1) for i in range(count)]
    return _YS[key]


def make(sp, shape, prec, plan=None):
    L, M, n = shape
    return sp.SparcOperator(L, M, n, ordering(sp, L, M, n), precision=prec, plan=plan)


def serial(sp, shape, prec, y, Pl, T, es=False, beta0=None, key=None):
    """One decode on a fresh single-lane operator: beta, iters, z, decisions.
    Cached under `key` (the reference of a case is computed once)."""
    full = None if key is None else (shape, prec, T, es, key)
    if full is not None and full in _REF:
        return _REF[full]
    op = make(sp, shape, prec, plan=("NO_LANES",))
    B = y.shape[0]
    op.reserve(B, 6)
    op.stage(y, Pl, beta0)
    op.run(B, T, early_stop=es, beta0=beta0 is not None)
    op.wait()
    beta, it = op.fetch(B)
    out = dict(beta=beta, iters=it, z=op.fetch_z(B), dec=op.decide(B))
    if full is not None:
        _REF[full] = out
    return out


def pipelined(op, steps, B=1):
    """bench.py's protocol, a new y per step: stage (unless y is None), run,
    decide_async(k % 2), collect step k - 1; nothing else synchronises.
    steps: (y, Pl, T, es, beta0) tuples.  Returns every step's decisions."""
    got = []
    for k, (y, Pl, T, es, b0) in enumerate(steps):
        if y is not None:
            op.stage(y, Pl, b0)
        op.run(B, T, early_stop=es, beta0=b0 is not None)
        op.decide_async(B, k % 2)
        if k > 0:
            got.append(op.decide_collect(B, (k - 1) % 2))
    got.append(op.decide_collect(B, (len(steps) - 1) % 2))
    return got


# ---- 1. a stream of different inputs ------------------------------------------

@pytest.mark.parametrize("es", [False, True])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", SHAPES)
def test_stream_of_inputs(sp, shape, prec, es):
    """Six different y through the ring, one step behind: every collected
    decision equals the serial decode's (a NO_LANES operator fed the same
    stream, and a fresh operator per input); after the last step fetch,
    fetch_z and iters are the last decode's."""
    L, M, n = shape
    T, Pl, ys = 5, power(L), inputs(*shape)
    steps = [(y, Pl, T, es, None) for y in ys]
    op = make(sp, shape, prec)
    op.reserve(1, 6)
    got = pipelined(op, steps)
    one = make(sp, shape, prec, plan=("NO_LANES",))
    one.reserve(1, 6)
    got1 = pipelined(one, steps)
    refs = [serial(sp, shape, prec, y, Pl, T, es, key=("y", i)) for i, y in enumerate(ys)]
    assert not np.array_equal(refs[0]["dec"], refs[1]["dec"])
    for k in range(len(ys)):
        assert np.array_equal(got[k], refs[k]["dec"]), k
        assert np.array_equal(got1[k], refs[k]["dec"]), k
    for o in (op, one):
        beta, it = o.fetch(1)
        assert np.array_equal(it, refs[-1]["iters"]) and np.array_equal(o.iters(1), refs[-1]["iters"])
        assert np.array_equal(beta, refs[-1]["beta"])
        assert np.array_equal(o.fetch_z(1), refs[-1]["z"])


# ---- 2. the same input run again ------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", SHAPES)
def test_same_input_rerun(sp, shape, prec):
    """Staged once, run four times: a run with no stage since the previous one
    decodes the same y again, on whichever lane (the lane that never saw the
    upload gets the device copy)."""
    L, M, n = shape
    T, Pl, y = 5, power(L), inputs(*shape)[0]
    ref = serial(sp, shape, prec, y, Pl, T, key=("y", 0))
    op = make(sp, shape, prec)
    op.reserve(1, 6)
    got = pipelined(op, [(y, Pl, T, False, None)] + [(None, Pl, T, False, None)] * 3)
    for k in range(4):
        assert np.array_equal(got[k], ref["dec"]), k
    beta, it = op.fetch(1)
    assert np.array_equal(beta, ref["beta"]) and np.array_equal(it, ref["iters"])


# ---- 3. no stale state across lanes ---------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", SHAPES)
def test_no_stale_state_across_lanes(sp, shape, prec):
    """T = 6, 1, 5 against y1 / y2 arranged so that each lane decodes odd and
    even T after the other input; a beta0 run between two pipelined ones (it
    stays on the current lane); a new Pl staged while a decode is in flight
    (the later run uses it, the earlier one is unharmed)."""
    L, M, n = shape
    Pl, Pl2 = power(L), power(L, 3.0)
    y = inputs(*shape)[:2]
    # lanes alternate from step 0: lane 0 sees (y1, 6) (y2, 5) (y1, 1) (y2, 6), lane 1 (y2, 1) (y1, 6) (y2, 5) (y1, 1)
    plan = [(0, 6), (1, 1), (1, 5), (0, 6), (0, 1), (1, 5), (1, 6), (0, 1)]
    rs = np.random.RandomState(9)
    b0 = np.zeros((1, L * M))
    b0[0, np.arange(L) * M + rs.randint(0, M, L)] = np.sqrt(n * Pl)
    steps = [(y[i], Pl, T, False, None) for i, T in plan]
    want = [serial(sp, shape, prec, y[i], Pl, T, key=("y", i)) for i, T in plan]
    # the beta0 run and two plain ones behind it
    steps += [(y[0], Pl, 5, False, b0), (y[1], Pl, 5, False, None), (y[0], Pl, 6, False, None)]
    want += [serial(sp, shape, prec, y[0], Pl, 5, beta0=b0, key=("b0", 0)),
             serial(sp, shape, prec, y[1], Pl, 5, key=("y", 1)), serial(sp, shape, prec, y[0], Pl, 6, key=("y", 0))]
    # a new power allocation while the previous decode is in flight
    steps += [(y[1], Pl2, 6, False, None), (y[0], Pl, 5, False, None)]
    want += [serial(sp, shape, prec, y[1], Pl2, 6, key=("P2", 1)), serial(sp, shape, prec, y[0], Pl, 5, key=("y", 0))]
    op = make(sp, shape, prec)
    op.reserve(1, 6)
    got = pipelined(op, steps)
    for k in range(len(steps)):
        assert np.array_equal(got[k], want[k]["dec"]), (k, steps[k][2])
    beta, it = op.fetch(1)
    assert np.array_equal(beta, want[-1]["beta"]) and np.array_equal(it, want[-1]["iters"])
    # the new power changes the estimate (the check above can tell the two allocations apart)
    assert not np.array_equal(want[-2]["beta"], serial(sp, shape, prec, y[1], Pl, 6, key=("y", 1))["beta"])


# ---- 4. reallocation ---------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_reallocation(sp, prec):
    """After both lanes have run: reserve with a larger T, then with B = 2.
    Decodes afterwards are correct (the second lane returns with the first
    pipelined step), and once both lanes exist the device byte count does not
    grow from run to run."""
    shape = SHAPES[0]
    L, M, n = shape
    Pl, ys = power(L), inputs(*shape)
    op = make(sp, shape, prec)
    op.reserve(1, 4)

    def check(B, T, tag):
        yb = [np.concatenate(ys[i:i + B]) for i in range(3)]
        steps = [(yk, Pl, T, False, None) for yk in yb]
        first = op.info()["device_bytes"]
        got = pipelined(op, steps, B)  # lane 1 appears with the first step issued behind an outstanding one
        size = op.info()["device_bytes"]
        lane = 2 * L * M * (4 if prec == "fp32" else 8) * B
        assert size - first >= lane, (tag, first, size)  # two estimate buffers at the least
        more = pipelined(op, steps, B) + pipelined(op, steps[:2], B)
        assert op.info()["device_bytes"] == size, tag
        refs = [serial(sp, shape, prec, yk, Pl, T, key=(tag, k)) for k, yk in enumerate(yb)]
        for k in range(3):
            assert np.array_equal(got[k], refs[k]["dec"]) and np.array_equal(more[k], refs[k]["dec"]), (tag, k)
        assert np.array_equal(more[3], refs[0]["dec"]) and np.array_equal(more[4], refs[1]["dec"]), tag
        beta, it = op.fetch(B)
        assert np.array_equal(beta, refs[1]["beta"]) and np.array_equal(it, refs[1]["iters"]), tag
        return size

    s0 = check(1, 4, "T4")
    op.reserve(1, 6)
    s1 = check(1, 6, "T6")
    op.reserve(2, 6)
    s2 = check(2, 6, "B2")
    assert s0 < s1 < s2


# ---- 5. lanes stay off where they must -----------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_lanes_stay_off(sp, prec):
    """A batched decode, an EAGER operator and a NO_LANES operator never get a
    second workspace (the byte count after the first run is the byte count
    after several pipelined ones) and give the default plan's results."""
    # batched: B = 5 at L = M = 64
    L, M, n, B, T = 64, 64, 384, 5, 5
    Pl = power(L)
    yb = np.concatenate(inputs(L, M, n, B))
    op = sp.SparcOperator(L, M, n, ordering(sp, L, M, n), precision=prec)
    assert op.plan(B)["section_kernel"] == "k_secb"
    op.reserve(B, T)
    op.stage(yb, Pl)
    outs, size = [], []
    for _ in range(4):
        op.run(B, T, early_stop=False)
        op.wait()
        outs.append(op.fetch(B)[0])
        size.append(op.info()["device_bytes"])
    assert size[0] == size[1] == size[2] == size[3], size  # (the first fetch sizes the staging buffer)
    ref = serial(sp, (L, M, n), prec, yb, Pl, T)
    assert all(np.array_equal(o, ref["beta"]) for o in outs)
    # one codeword: EAGER and NO_LANES against the default plan (lanes on)
    shape = SHAPES[0]
    Pl, ys = power(shape[0]), inputs(*shape)[:3]
    steps = [(y, Pl, T, False, None) for y in ys]
    dflt = make(sp, shape, prec)
    dflt.reserve(1, T)
    want = pipelined(dflt, steps)
    dsize = dflt.info()["device_bytes"]
    wbeta = dflt.fetch(1)[0]
    # lone decodes (run, wait: nothing outstanding at the next run) stay on one lane under the default plan too
    lone = make(sp, shape, prec)
    lone.reserve(1, T)
    sizes = []
    for y in ys:
        lone.stage(y, Pl)
        lone.run(1, T, early_stop=False)
        lone.wait()
        assert np.array_equal(lone.decide(1), want[len(sizes)])
        sizes.append(lone.info()["device_bytes"])
    assert sizes[0] == sizes[1] == sizes[2] and dsize - sizes[2] >= 2 * shape[0] * shape[1] * 4, (sizes, dsize)
    for plan in ("EAGER", "NO_LANES"):
        o = make(sp, shape, prec, plan=(plan,))
        o.reserve(1, T)
        o.stage(ys[0], Pl)
        o.run(1, T, early_stop=False)
        o.wait()
        size = o.info()["device_bytes"]
        got = pipelined(o, steps)
        assert o.info()["device_bytes"] == size, plan
        # the default plan did create lane 1: two more estimate buffers at the least
        assert dsize - size >= 2 * shape[0] * shape[1] * (4 if prec == "fp32" else 8), (plan, dsize, size)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (plan, k)
        assert np.array_equal(o.fetch(1)[0], wbeta), plan


# ---- 6. B = 3 on the small-batch path ---------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_three_codewords_pipelined(sp, prec):
    """The ring test's shape (L = 64, M = 512, n = 576, B = 3), pipelined."""
    shape, B, T = (64, 512, 576), 3, 4
    Pl, ys = power(shape[0]), inputs(*shape, count=9)
    yb = [np.concatenate(ys[3 * k:3 * k + 3]) for k in range(3)]
    op = make(sp, shape, prec)
    op.reserve(B, T)
    got = pipelined(op, [(y, Pl, T, False, None) for y in yb] + [(None, Pl, T, False, None)], B)
    refs = [serial(sp, shape, prec, y, Pl, T, key=("b3", k)) for k, y in enumerate(yb)]
    for k in range(3):
        assert np.array_equal(got[k], refs[k]["dec"]), k
    assert np.array_equal(got[3], refs[2]["dec"])
    beta, it = op.fetch(B)
    assert np.array_equal(beta, refs[2]["beta"]) and np.array_equal(it, refs[2]["iters"])
    assert np.array_equal(op.fetch_z(B), refs[2]["z"])


# ---- 7. a stage with no run behind it ------------------------------------------------------

@pytest.mark.parametrize("outstanding", [False, True])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(64, 512, 581), (256, 256, 2048)])
def test_stage_then_fetch_y_then_run(sp, shape, prec, outstanding):
    """Two pipelined steps (the second ran on lane 1, which stays current),
    then a new y staged with no run behind it: fetch_y returns the staged word
    (binary32: its float rounding), and run, wait, fetch give the serial
    NO_LANES decode of that word bit for bit.  Again with beta0 given, which
    keeps the next run on the current lane.  `outstanding`: step 1's decisions
    are collected only after the run, so the stage without beta0 writes the
    lane that is not current and fetch_y has to bring the word over."""
    L, M, n = shape
    T, Pl, ys = 4, power(L), inputs(*shape)
    wt = np.float32 if prec == "fp32" else np.float64
    b0 = np.zeros((1, L * M))
    b0[0, np.arange(L) * M + np.random.RandomState(9).randint(0, M, L)] = np.sqrt(n * Pl)
    for beta0, key in ((None, ("y", 2)), (b0, ("b0", 2))):
        op = make(sp, shape, prec)
        op.reserve(1, 6)
        dec = [None, None]
        for k in range(2):
            op.stage(ys[k], Pl)
            op.run(1, T, early_stop=False)
            op.decide_async(1, k)
            if k > 0:
                dec[0] = op.decide_collect(1, 0)
        if not outstanding:
            dec[1] = op.decide_collect(1, 1)
        op.stage(ys[2], Pl, beta0)
        assert np.array_equal(op.fetch_y(1), ys[2].astype(wt).astype(np.float64)), key
        op.run(1, T, early_stop=False, beta0=beta0 is not None)
        op.wait()
        beta, it = op.fetch(1)
        if outstanding:
            dec[1] = op.decide_collect(1, 1)
        ref = serial(sp, shape, prec, ys[2], Pl, T, beta0=beta0, key=key)
        assert np.array_equal(beta, ref["beta"]) and np.array_equal(it, ref["iters"]), key
        assert np.array_equal(op.fetch_z(1), ref["z"]) and np.array_equal(op.decide(1), ref["dec"]), key
        for k in range(2):  # the steps before the stage are unharmed
            assert np.array_equal(dec[k], serial(sp, shape, prec, ys[k], Pl, T, key=("y", k))["dec"]), (key, k)
    assert not np.array_equal(serial(sp, shape, prec, ys[2], Pl, T, key=("y", 2))["beta"],
                              serial(sp, shape, prec, ys[2], Pl, T, beta0=b0, key=("b0", 2))["beta"])
