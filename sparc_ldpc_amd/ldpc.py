"""LDPC outer code of the joint decoder: mirror of the reference's ``ldpc.code``
(ldpc/py/ldpc.py:6-943) with belief propagation running on the GPU.

``code(standard, rate, z, ptype)`` builds the same Tanner graph
(``vdeg``, ``cdeg``, ``intrlv``: identical arrays, ldpc.py:694-786) from the
same base matrices (``data/protographs.json``), encodes systematically
(ldpc.py:790-850) and decodes through ``libldpc_bp.so``
(include/ldpc_bp.h), the HIP replacement of ``bin/c_ldpc.so``.  The decoder
returns ``(app, it)`` like ldpc.py:855-930; ``decode_batch`` decodes many
words of one code in one launch.  There is no CPU decoder: without the
library or a HIP device, decoding raises.
"""
from __future__ import annotations

import ctypes as ct
import functools
import json
import os

import numpy as np

MAX_ITCOUNT = 200  # ldpc.py:4 / c_ldpc.c:7

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LDPC_BP_LIB") or os.path.join(_HERE, "libldpc_bp.so")

LB_SUMPROD2, LB_SUMPROD, LB_MINSUM, LB_LAYERED_SUMPROD2, LB_LAYERED_MINSUM = 0, 1, 2, 3, 4
LB_F32 = 0x100  # precision flag OR-ed into a layered type: binary32 messages
_ALGOS = {"sumprod2": LB_SUMPROD2, "sumprod": LB_SUMPROD, "minsum": LB_MINSUM,
          "layered_sumprod2": LB_LAYERED_SUMPROD2, "layered_minsum": LB_LAYERED_MINSUM,
          "layered_sumprod2_f32": LB_LAYERED_SUMPROD2 | LB_F32, "layered_minsum_f32": LB_LAYERED_MINSUM | LB_F32}
LB_FIXED = 0x400  # arithmetic flag OR-ed into LB_LAYERED_MINSUM: saturating integers (the quant keyword)
FIXED_DEFAULT = (2, 6, 8)  # frac_bits, msg_bits, app_bits of quant=True (lb_set_fixed's defaults)
_REFERENCE_ALGOS = ("sumprod2", "sumprod", "minsum")  # code.decode's names (ldpc.py:855-930)
_CHANNELS = {"awgn": 0, "bsc": 1}  # lb_mc_run / lb_draw_blocks kinds
STREAM_CHUNK = 4096  # blocks per chunk of code.mc_stream_seeds

# Every symbol include/ldpc_bp.h declares (tests check the export table).
EXPORTS = (
    "sumprod", "sumprod2", "minsum", "Lxor", "Lxfb",
    "lb_create", "lb_destroy", "lb_decode", "lb_decode_device", "lb_stage", "lb_run", "lb_wait",
    "lb_fetch", "lb_run_event_ms", "lb_info", "lb_device_count", "lb_last_error", "lb_version",
    "lb_buffers", "lb_set_tail", "lb_set_layers", "lb_layer_info", "lb_layer_info_ex",
    "lb_draw_blocks", "lb_mc_set_code", "lb_encode", "lb_mc_run", "lb_mc_run_seeds", "lb_draw_blocks_device",
    "lb_mc_stream_seeds", "lb_set_fixed", "lb_fixed_info", "lb_joint_draw", "lb_joint_fetch",
)

_P, _I, _D = ct.c_void_p, ct.c_int, ct.POINTER(ct.c_double)
_LP = ct.POINTER(ct.c_long)
_U8, _IP = ct.POINTER(ct.c_uint8), ct.POINTER(ct.c_int)
_SIG = {
    "sumprod": (_I, [_D, _LP, _LP, _LP, _I, _I, _I, _D]),
    "sumprod2": (_I, [_D, _LP, _LP, _LP, _I, _I, _I, _D]),
    "minsum": (_I, [_D, _LP, _LP, _LP, _I, _I, _I, _D, ct.c_double]),
    "Lxor": (ct.c_double, [ct.c_double, ct.c_double, _I]),
    "Lxfb": (ct.c_double, [_D, ct.c_long, _I]),
    "lb_create": (_I, [ct.POINTER(_P), _LP, _LP, _LP, _I, _I, _I, _I]),
    "lb_destroy": (None, [_P]),
    "lb_decode": (_I, [_P, _I, _D, _D, ct.POINTER(ct.c_int), _I, ct.c_double, _I]),
    "lb_decode_device": (_I, [_P, _I, _P, _P, _P, _I, ct.c_double, _I]),
    "lb_stage": (_I, [_P, _I, _D]),
    "lb_buffers": (_I, [_P, _I, ct.POINTER(_P), ct.POINTER(_P), ct.POINTER(_P)]),
    "lb_run": (_I, [_P, _I, _I, ct.c_double, _I]),
    "lb_wait": (_I, [_P]),
    "lb_fetch": (_I, [_P, _I, _D, ct.POINTER(ct.c_int)]),
    "lb_run_event_ms": (ct.c_double, [_P]),
    "lb_info": (_I, [_P, ct.POINTER(ct.c_int64)]),
    "lb_set_tail": (_I, [_P, _I]),
    "lb_set_layers": (_I, [_P, _I, _IP]),
    "lb_layer_info": (_I, [_P, ct.POINTER(ct.c_int64)]),
    "lb_layer_info_ex": (_I, [_P, _I, ct.POINTER(ct.c_int64)]),
    "lb_set_fixed": (_I, [_P, _I, _I, _I]),
    "lb_fixed_info": (_I, [_P, ct.POINTER(ct.c_int64)]),
    "lb_device_count": (_I, []),
    "lb_last_error": (ct.c_char_p, []),
    "lb_version": (ct.c_char_p, []),
    "lb_draw_blocks": (_I, [ct.POINTER(ct.c_uint32), _I, _I, _I, _I, _U8, _D, _I]),
    "lb_mc_set_code": (_I, [_P, _IP, _I, _I, _I]),
    "lb_encode": (_I, [_P, _I, _U8, _U8]),
    "lb_mc_run": (_I, [_P, _I, _U8, _D, ct.c_double, _I, _I, _I, ct.c_double, _I, _IP, _IP]),
    "lb_mc_run_seeds": (_I, [_P, _I, ct.POINTER(ct.c_uint32), _I, ct.c_double, _I, _I, _I, ct.c_double, _I, _IP,
                             _IP]),
    "lb_draw_blocks_device": (_I, [_P, ct.POINTER(ct.c_uint32), _I, _I, _I, _I, _U8, _D]),
    "lb_mc_stream_seeds": (_I, [_P, _I, ct.POINTER(ct.c_uint32), _I, ct.c_double, _I, _I, _I, _I, _I, ct.c_double,
                                _I, _IP, _IP, ct.POINTER(ct.c_int64)]),
    "lb_joint_draw": (_I, [_P, _I, ct.POINTER(ct.c_uint32), _I, _I, _I, ct.c_double, ct.POINTER(_P), ct.POINTER(_P),
                           _D]),
    "lb_joint_fetch": (_I, [_P, _I, _U8, _D]),
}

_lib = None


class LdpcBpError(RuntimeError):
    """A negative status from libldpc_bp.so."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"libldpc_bp error {code}: {msg}")
        self.code = code


def load_bp_library(path: str = LIB_PATH) -> ct.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with __graft_entry__.build() "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = ct.CDLL(path)
    for name, (res, args) in _SIG.items():
        fn = getattr(lib, name, None)
        if fn is None:  # an older build (A/B runs): the entry point stays absent
            continue
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _layered_entry(name):
    """An entry point of the layered decoder; an older libldpc_bp.so has none."""
    fn = getattr(load_bp_library(), name, None)
    if fn is None:
        raise LdpcBpError(-5, f"this libldpc_bp.so has no layered decoder ({name})")
    return fn


def _quant_widths(quant, dectype):
    """The (frac_bits, msg_bits, app_bits) a ``quant`` keyword asks for, or None:
    None: floating point as ever; True: FIXED_DEFAULT; a triple: those widths.
    ValueError unless the decoder type is "layered_minsum" (needs no device)."""
    if quant is None:
        return None
    if dectype != "layered_minsum":
        raise ValueError('quant (fixed-point arithmetic) goes with dectype="layered_minsum" only')
    if quant is True:
        return FIXED_DEFAULT
    try:
        f, m, a = (int(x) for x in quant)
    except (TypeError, ValueError):
        raise ValueError("quant must be None, True or (frac_bits, msg_bits, app_bits)") from None
    return f, m, a


def _check(rc: int) -> None:
    if rc < 0:
        msg = load_bp_library().lb_last_error().decode(errors="replace")
        if rc == -1:
            raise AssertionError(msg)
        raise LdpcBpError(rc, msg)


@functools.lru_cache(maxsize=None)
def _protographs():
    with open(os.path.join(_HERE, "data", "protographs.json")) as fh:
        return json.load(fh)["protographs"]


def assign_proto(standard, rate, z, ptype="A"):
    """Base matrix for (standard, rate[, ptype / z]) — ldpc.py:26-663, same errors."""
    tab = _protographs()
    if standard == "802.11n":
        if z not in (27, 54, 81):
            raise NameError("802.11n invalid z (must be 27,54 or 81)")
        by_rate = tab["802.11n"][str(z)]
        if rate not in by_rate:
            raise UnboundLocalError(f"no 802.11n protograph for rate {rate!r}")
        return np.array(by_rate[rate], dtype=np.int64)
    if standard not in tab["z_free"]:
        raise NameError("IEEE standard unknown")
    by_rate = tab["z_free"][standard]
    if rate not in by_rate:
        raise UnboundLocalError(f"no {standard} protograph for rate {rate!r}")
    by_type = by_rate[rate]
    if ptype not in by_type:
        if len(by_type) == 1:  # ptype is ignored for single-type rates (ldpc.py:43-45)
            return np.array(next(iter(by_type.values())), dtype=np.int64)
        raise UnboundLocalError(f"no {standard} rate {rate} protograph of type {ptype!r}")
    return np.array(by_type[ptype], dtype=np.int64)


def tanner_graph(proto: np.ndarray, z: int):
    """(vdeg, cdeg, intrlv) — the arrays of ldpc.py:694-786.

    The reference assigns ports while walking the protograph row by row
    (np.nonzero order), so check node (r, k)'s ports follow the columns of
    row r and variable node (c, k')'s ports follow the rows of column c.  With
    those two ranks the interleaver is written directly: entry (r, c) with
    shift s links check r*z+k to variable c*z+(k+s)%z."""
    proto = np.asarray(proto, dtype=np.int64)
    on = proto != -1
    cdeg = np.repeat(on.sum(1), z).astype(np.int64)
    vdeg = np.repeat(on.sum(0), z).astype(np.int64)
    cfirst = np.concatenate([[0], np.cumsum(cdeg)[:-1]])
    vfirst = np.concatenate([[0], np.cumsum(vdeg)[:-1]])
    cport = np.cumsum(on, 1) - 1
    vport = np.cumsum(on, 0) - 1
    r, c = np.nonzero(on)
    k = np.arange(z)[None, :]
    chk = r[:, None] * z + k
    var = c[:, None] * z + (k + proto[r, c][:, None]) % z
    intrlv = np.empty(int(cdeg.sum()), dtype=np.int64)
    intrlv[(vfirst[var] + vport[r, c][:, None]).ravel()] = (cfirst[chk] + cport[r, c][:, None]).ravel()
    return vdeg, cdeg, intrlv


def encode_batch(proto: np.ndarray, z: int, U) -> np.ndarray:
    """Systematic encoding of B information words (rows of U) — ldpc.py:790-850.

    Works on (B, Np, z) blocks: the systematic syndromes p_j, their sum gives
    the first parity block (after undoing the single surviving shift of column
    Kp), then the dual-diagonal recursion yields the remaining parity blocks."""
    proto = np.asarray(proto, dtype=np.int64)
    Mp, Np = proto.shape
    Kp = Np - Mp
    U = np.atleast_2d(np.asarray(U, dtype=np.int64))
    if U.shape[1] != Kp * z:
        raise NameError("information word length not compatible with proto and z")
    B = U.shape[0]
    x = np.zeros((B, Np, z), dtype=np.int64)
    x[:, :Kp] = U.reshape(B, Kp, z)
    p = np.zeros((B, Mp, z), dtype=np.int64)
    for j in range(Mp):
        for k in np.nonzero(proto[j, :Kp] != -1)[0]:
            p[:, j] ^= np.roll(x[:, k], -proto[j, k], axis=-1)
    col = proto[:, Kp]
    shifts = np.bincount(col[col != -1] % z, minlength=z) % 2
    nz = np.nonzero(shifts)[0]
    if len(nz) != 1:
        raise NameError("The offsets in colum Kp+1 of proto do not add to a single offset")
    x[:, Kp] = np.roll(np.bitwise_xor.reduce(p, axis=1), nz[0], axis=-1)
    for j in range(Mp - 1):
        m = Kp + j + 1
        acc = p[:, j].copy()
        for k in np.nonzero(proto[j, Kp:m] != -1)[0]:
            acc ^= np.roll(x[:, Kp + k], -proto[j, Kp + k], axis=-1)
        x[:, m] = acc
    return x.reshape(B, Np * z)


class code:
    """Drop-in for ``ldpc.code`` (ldpc/py/ldpc.py:6-24): same attributes
    (standard, rate, z, ptype, proto, vdeg, cdeg, intrlv, Nv, Nc, Nmsg, N, K)
    and methods (assign_proto, pcmat, prepare_decoder, encode, decode, Lxor,
    Lxfb), plus ``encode_batch`` / ``decode_batch`` for Monte-Carlo and the
    device-side ``encode_device`` / ``mc_blocks`` (encode, channel, decode and
    error count without a host round trip).

    ``decode_batch``, ``run_buffers``, ``mc_blocks`` and ``mc_blocks_seeds``
    also take dectype "layered_sumprod2" / "layered_minsum": the layered
    schedule over the protograph rows (include/ldpc_bp.h, lb_set_layers), whose
    ``it`` counts sweeps; and "layered_sumprod2_f32" / "layered_minsum_f32":
    the same schedule on binary32 messages (LB_F32; CH and app stay float64,
    CH is clamped to +-2**100 on load).  ``mc_stream_seeds`` runs
    ``mc_blocks_seeds``' blocks, with a layered dectype, as a stream of refilled
    decoder slots with an optional stopping rule (lb_mc_stream_seeds).

    These five also take ``quant`` with dectype "layered_minsum": the
    fixed-point decoder (LB_FIXED, include/ldpc_bp.h), layered normalised
    min-sum on saturating integers.  None: floating point as ever; True:
    FIXED_DEFAULT; (frac_bits, msg_bits, app_bits): those widths.  With any
    other dectype it is a ValueError.  app stays float64 and holds
    int * 2**-frac_bits exactly; ``decode`` (the reference's signature) does
    not take it."""

    def __init__(self, standard="802.11n", rate="1/2", z=27, ptype="A", device=None):
        self.standard = standard
        self.rate = rate
        self.z = z
        self.ptype = ptype
        self.proto = self.assign_proto()
        vdeg, cdeg, intrlv = self.prepare_decoder()
        self.vdeg = vdeg
        self.cdeg = cdeg
        self.intrlv = intrlv
        self.Nv = len(vdeg)
        self.Nc = len(cdeg)
        self.Nmsg = len(intrlv)
        self.N = self.Nv
        self.K = self.Nv - self.Nc
        self._device = device
        self._ctx = None
        self._encoder_set = False
        self._layers_set = False
        self._joint_shape = (0, 0, 0)  # reps, message bits and noise values a rep of the last joint_draw

    # -- construction ---------------------------------------------------------
    def assign_proto(self):
        return assign_proto(self.standard, self.rate, self.z, self.ptype)

    def pcmat(self):
        """Dense parity-check matrix (ldpc.py:666-691)."""
        z = self.z
        H = np.zeros((z * self.proto.shape[0], z * self.proto.shape[1]), dtype=int)
        eye = np.eye(z, dtype=int)
        for r, c in zip(*np.nonzero(self.proto != -1)):
            H[r * z:(r + 1) * z, c * z:(c + 1) * z] = np.roll(eye, self.proto[r, c] % z, 1)
        return H

    def prepare_decoder(self):
        return tanner_graph(self.proto, self.z)

    def encode(self, info):
        return encode_batch(self.proto, self.z, np.asarray(info).reshape(1, -1))[0]

    def encode_batch(self, U):
        return encode_batch(self.proto, self.z, U)

    # -- decoding (GPU) ---------------------------------------------------------
    def _context(self):
        if self._ctx is None:
            lib = load_bp_library()
            dev = self._device
            if dev is None:
                ndev = lib.lb_device_count()
                if ndev <= 0:
                    raise LdpcBpError(-6, "no HIP device visible (MI355X required; no CPU decoder)")
                env = os.environ.get("SPARC_AMP_DEVICE", os.environ.get("LOCAL_RANK", "0"))
                dev = int(env) if 0 <= int(env) < ndev else 0
            ctx = ct.c_void_p()
            v = np.ascontiguousarray(self.vdeg, dtype=np.int64)
            c = np.ascontiguousarray(self.cdeg, dtype=np.int64)
            il = np.ascontiguousarray(self.intrlv, dtype=np.int64)
            _check(lib.lb_create(ct.byref(ctx), v.ctypes.data_as(_LP), c.ctypes.data_as(_LP),
                                 il.ctypes.data_as(_LP), self.Nv, self.Nc, self.Nmsg, int(dev)))
            self._ctx = ctx
        return self._ctx

    def _algo(self, dectype, quant=None):
        """The library's number of a decoder type; a layered one sets the
        context's layers (the protograph rows) on first use.  ``quant``: the
        context's fixed-point widths are set and LB_FIXED is OR-ed in."""
        if dectype not in _ALGOS:
            raise NameError("Decoder type unknonwn")
        widths = _quant_widths(quant, dectype)
        if dectype.startswith("layered_") and not self._layers_set:
            self.set_layers(np.arange(0, self.Nc + 1, self.z))
        if widths is None:
            return _ALGOS[dectype]
        self.set_fixed(*widths)
        return _ALGOS[dectype] | LB_FIXED

    def set_fixed(self, frac_bits=FIXED_DEFAULT[0], msg_bits=FIXED_DEFAULT[1], app_bits=FIXED_DEFAULT[2]):
        """The widths of the fixed-point decoder for the decodes that follow
        (lb_set_fixed: frac_bits 0..8, msg_bits 2..8, app_bits msg_bits..16;
        AssertionError otherwise, and the widths stay as they were)."""
        _check(_layered_entry("lb_set_fixed")(self._context(), int(frac_bits), int(msg_bits), int(app_bits)))

    def fixed_info(self):
        """lb_fixed_info: the widths, and (0 before the layers are set) threads
        per workgroup, lanes per check, dynamic LDS bytes, workgroups resident
        on a CU and whether the int16 / int8 image fits LDS."""
        out = (ct.c_int64 * 8)()
        _check(_layered_entry("lb_fixed_info")(self._context(), out))
        keys = ("frac_bits", "msg_bits", "app_bits", "threads", "lanes", "lds_bytes", "resident", "fits")
        return dict(zip(keys, list(out)))

    def set_layers(self, first_check):
        """Layer l = the checks first_check[l] .. first_check[l+1]-1
        (lb_set_layers; LdpcBpError -4 when they do not increase strictly from
        0 to Nc or a variable occurs twice in a layer)."""
        fc = np.ascontiguousarray(first_check, dtype=np.intc)
        _check(_layered_entry("lb_set_layers")(self._context(), len(fc) - 1, fc.ctypes.data_as(_IP)))
        self._layers_set = True

    def layer_info(self, precision="f64"):
        """lb_layer_info: layers, the largest layer's checks, where the layered
        decoder keeps its messages (2: r and app in LDS, 1: app in LDS, 0: HBM)
        and its threads per workgroup.  precision="f32" (lb_layer_info_ex) gives
        these for the binary32 decoders and adds lds_bytes (dynamic LDS of a
        workgroup), resident / resident_minsum (workgroups of the sumprod2 /
        minsum instance a CU holds at once) and message_bytes."""
        if precision not in ("f64", "f32"):
            raise ValueError('precision must be "f64" or "f32"')
        keys = ("nlayers", "max_layer", "lds_messages", "threads")
        if precision == "f64":
            out = (ct.c_int64 * 4)()
            _check(_layered_entry("lb_layer_info")(self._context(), out))
            return dict(zip(keys, list(out)))
        out = (ct.c_int64 * 8)()
        _check(_layered_entry("lb_layer_info_ex")(self._context(), 1, out))
        return dict(zip(keys + ("lds_bytes", "resident", "resident_minsum", "message_bytes"), list(out)))

    def decode_batch(self, CH, dectype="sumprod2", corr_factor=0.7, max_iter=MAX_ITCOUNT, quant=None):
        """Decode B words (rows of CH, channel LLRs) -> (app (B, N) float64, it (B,) int)."""
        algo = self._algo(dectype, quant)
        CH = np.ascontiguousarray(np.atleast_2d(CH), dtype=np.float64)
        if CH.shape[1] != self.Nv:
            raise NameError("Channel inputs not consistent with variable degrees")
        B = CH.shape[0]
        app = np.empty((B, self.Nv), dtype=np.float64)
        it = np.empty(B, dtype=np.intc)
        lib = load_bp_library()
        _check(lib.lb_decode(self._context(), B, CH.ctypes.data_as(_D), app.ctypes.data_as(_D),
                             it.ctypes.data_as(ct.POINTER(ct.c_int)), algo,
                             float(corr_factor), int(max_iter)))
        return app, it.astype(np.int64)

    # -- device-side Monte-Carlo (csrc/ldpc_mc.hip) ------------------------------
    def _set_encoder(self):
        """Upload the base matrix to the context once (lb_mc_set_code); like
        encode_batch, NameError when column Kp does not reduce to one offset."""
        if self._encoder_set:
            return
        proto = np.ascontiguousarray(self.proto, dtype=np.intc)
        Mp, Np = proto.shape
        lib = load_bp_library()
        rc = lib.lb_mc_set_code(self._context(), proto.ctypes.data_as(_IP), Mp, Np, int(self.z))
        if rc == -1 and b"single offset" in lib.lb_last_error():
            raise NameError("The offsets in colum Kp+1 of proto do not add to a single offset")
        _check(rc)
        self._encoder_set = True

    def encode_device(self, U):
        """encode_batch on the GPU (k_mc_prep's encoder): rows of 0/1 bits -> (B, N) uint8."""
        U = np.atleast_2d(np.asarray(U))
        if U.shape[1] != self.K:
            raise NameError("information word length not compatible with proto and z")
        if U.size and (U.min() < 0 or U.max() > 1):
            raise ValueError("information bits must be 0 or 1")
        U = np.ascontiguousarray(U, dtype=np.uint8)
        self._set_encoder()
        X = np.empty((U.shape[0], self.N), dtype=np.uint8)
        _check(load_bp_library().lb_encode(self._context(), U.shape[0], U.ctypes.data_as(_U8), X.ctypes.data_as(_U8)))
        return X

    def mc_blocks(self, u, w, a, channel="awgn", batch=1024, dectype="sumprod2", corr_factor=0.7,
                  max_iter=MAX_ITCOUNT, quant=None):
        """Blocks through the device pipeline (lb_mc_run): u (B, K) 0/1 uint8
        information bits (None: the all-zero word), w (B, N) float64 draws
        (randn for "awgn", random_sample for "bsc"), a = sigma or p.  Per block:
        encode, ch = (2/sigma**2) * ((1 - 2x) + sigma*w) or -/+ log((1-p)/p)
        where w < p / elsewhere, decode, count.  Returns int64 (bit_errors,
        iters); only those come back from the device."""
        algo = self._algo(dectype, quant)
        if channel not in _CHANNELS:
            raise ValueError(f"channel must be one of {sorted(_CHANNELS)}")
        w = np.ascontiguousarray(np.atleast_2d(w), dtype=np.float64)
        if w.shape[1] != self.N:
            raise NameError("Channel inputs not consistent with variable degrees")
        B = w.shape[0]
        up = None
        if u is not None:
            if channel == "bsc":
                raise ValueError("the BSC simulation sends the all-zero word (u must be None)")
            u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.uint8)
            if u.shape != (B, self.K):
                raise NameError("information word length not compatible with proto and z")
            self._set_encoder()
            up = u.ctypes.data_as(_U8)
        errs = np.empty(B, dtype=np.intc)
        it = np.empty(B, dtype=np.intc)
        _check(load_bp_library().lb_mc_run(self._context(), B, up, w.ctypes.data_as(_D), float(a),
                                            _CHANNELS[channel], int(batch), algo, float(corr_factor),
                                            int(max_iter), errs.ctypes.data_as(_IP), it.ctypes.data_as(_IP)))
        return errs.astype(np.int64), it.astype(np.int64)

    def _seeded(self, seeds, channel, dectype, quant):
        """What mc_blocks_seeds and mc_stream_seeds start from: the decoder's
        number, the seeds as uint32, K (ldpc_mc.info_bits; the encoder set where
        bits are drawn) and the two result arrays."""
        from .ldpc_mc import _seed_array, info_bits
        algo = self._algo(dectype, quant)
        if channel not in _CHANNELS:
            raise ValueError(f"channel must be one of {sorted(_CHANNELS)}")
        seeds = _seed_array(seeds)
        K = info_bits(self, channel)
        if K:
            self._set_encoder()
        return algo, seeds, K, np.empty(len(seeds), dtype=np.intc), np.empty(len(seeds), dtype=np.intc)

    def mc_blocks_seeds(self, seeds, a, channel="awgn", batch=1024, dectype="sumprod2", corr_factor=0.7,
                        max_iter=MAX_ITCOUNT, quant=None):
        """mc_blocks on blocks drawn on the device from their seeds
        (lb_mc_run_seeds; the blocks of ldpc_mc.draw_blocks_device): only the
        seeds go up.  The information bits are drawn where ldpc_mc.info_bits
        says the reference encodes, else the all-zero word is sent.  Returns
        int64 (bit_errors, iters) in seed order."""
        algo, seeds, K, errs, it = self._seeded(seeds, channel, dectype, quant)
        _check(load_bp_library().lb_mc_run_seeds(self._context(), len(seeds),
                                                  seeds.ctypes.data_as(ct.POINTER(ct.c_uint32)), K, float(a),
                                                  _CHANNELS[channel], int(batch), algo, float(corr_factor),
                                                  int(max_iter), errs.ctypes.data_as(_IP), it.ctypes.data_as(_IP)))
        return errs.astype(np.int64), it.astype(np.int64)

    def mc_stream_seeds(self, seeds, a, channel="awgn", chunk=STREAM_CHUNK, dectype="layered_sumprod2",
                        corr_factor=0.7, max_iter=MAX_ITCOUNT, min_errors=0, slots=0, quant=None):
        """mc_blocks_seeds as a stream of refilled decoder slots
        (lb_mc_stream_seeds; layered decoders only): per chunk of ``chunk``
        blocks one persistent kernel of ``slots`` workgroups (0: what the
        device holds at once) that takes the blocks by ticket, decodes and
        counts them; two chunks in flight on two lanes.  Per block the same
        (bit_errors, iters) as mc_blocks_seeds.  min_errors > 0: the stopping
        rule of harness.ber_point on the device and the host; blocks behind
        the stopping block may come back undecoded (iters = -1, bit_errors
        = 0).  Returns int64 (bit_errors, iters) in seed order and info =
        dict(used: the blocks the rule consumes (all of them without a rule),
        decoded, slots, chunks)."""
        # (a flooding type: LdpcBpError -5 from the library)
        algo, seeds, K, errs, it = self._seeded(seeds, channel, dectype, quant)
        out = (ct.c_int64 * 4)()
        _check(_layered_entry("lb_mc_stream_seeds")(
            self._context(), len(seeds), seeds.ctypes.data_as(ct.POINTER(ct.c_uint32)), K, float(a),
            _CHANNELS[channel], int(chunk), int(slots), int(min_errors), algo, float(corr_factor), int(max_iter),
            errs.ctypes.data_as(_IP), it.ctypes.data_as(_IP), out))
        return errs.astype(np.int64), it.astype(np.int64), dict(zip(("used", "decoded", "slots", "chunks"), list(out)))

    def joint_draw(self, seeds, U, n, sigma):
        """The reps of the joint SPARC + LDPC simulators drawn and encoded on the
        device from their seeds (lb_joint_draw): per seed randint(0, 2, K)
        protected bits, randint(0, 2, U) unprotected bits, randn(n) * sigma, the
        protected bits encoded.  Seeds outside [0, 2**32) raise ValueError (no
        masking).  Returns the device pointers (message bits (B, U + N) uint8:
        unprotected bits then codeword; noise (B, n) float64), valid until the
        next joint_draw of this code, and the device milliseconds."""
        from .operators import seed_array
        seeds = seed_array(seeds)
        self._set_encoder()
        bits, noise = ct.c_void_p(), ct.c_void_p()
        ms = ct.c_double(0.0)
        _check(load_bp_library().lb_joint_draw(self._context(), len(seeds),
                                               seeds.ctypes.data_as(ct.POINTER(ct.c_uint32)), self.K, int(U), int(n),
                                               float(sigma), ct.byref(bits), ct.byref(noise), ct.byref(ms)))
        self._joint_shape = (len(seeds), int(U) + self.N, int(n))
        return bits.value, noise.value, float(ms.value)

    def joint_fetch(self, bits=True, noise=True):
        """The reps of the last joint_draw copied back (lb_joint_fetch):
        (message bits (B, U + N) uint8 or None, noise (B, n) float64 or None)."""
        B, nb, n = self._joint_shape
        b = np.empty((B, nb), dtype=np.uint8) if bits else None
        w = np.empty((B, n)) if noise else None
        _check(load_bp_library().lb_joint_fetch(self._context(), B, None if b is None else b.ctypes.data_as(_U8),
                                                None if w is None else w.ctypes.data_as(_D)))
        return b, w

    def mc_event_ms(self):
        """Device milliseconds of the last mc_blocks / run_buffers (events on the context's stream)."""
        return float(load_bp_library().lb_run_event_ms(self._context()))

    def device_buffers(self, B):
        """Device pointers (ch, app, iters) of the decoder's buffers for B words."""
        ch, app, it = ct.c_void_p(), ct.c_void_p(), ct.c_void_p()
        _check(load_bp_library().lb_buffers(self._context(), int(B), ct.byref(ch), ct.byref(app), ct.byref(it)))
        return ch.value, app.value, it.value

    def run_buffers(self, B, dectype="sumprod2", corr_factor=0.7, max_iter=MAX_ITCOUNT, quant=None):
        """Decode the B words in the device ch buffer into the app buffer (blocking)."""
        if dectype not in _ALGOS:
            raise KeyError(dectype)  # as before the layered names
        algo = self._algo(dectype, quant)
        lib = load_bp_library()
        _check(lib.lb_run(self._context(), int(B), algo, float(corr_factor), int(max_iter)))
        _check(lib.lb_wait(self._context()))

    def fetch_buffers(self, B, app=True):
        """(app (B, N) or None, iters (B,)) from the device buffers."""
        a = np.empty((B, self.Nv)) if app else None
        it = np.empty(B, dtype=np.intc)
        _check(load_bp_library().lb_fetch(self._context(), int(B), None if a is None else a.ctypes.data_as(_D),
                                          it.ctypes.data_as(ct.POINTER(ct.c_int))))
        return a, it.astype(np.int64)

    def decode(self, ch, dectype="sumprod2", corr_factor=0.7):
        """ldpc.py:855-930: (app, it) for one word of channel LLRs."""
        if dectype not in _REFERENCE_ALGOS:
            raise NameError("Decoder type unknonwn")
        ch = np.asarray(ch, dtype=np.float64).reshape(-1)
        if len(ch) != len(self.vdeg):
            raise NameError("Channel inputs not consistent with variable degrees")
        app, it = self.decode_batch(ch[None, :], dectype, corr_factor)
        return app[0], int(it[0])

    def info(self):
        out = (ct.c_int64 * 10)()
        _check(load_bp_library().lb_info(self._context(), out))
        keys = ("Nv", "Nc", "Nmsg", "max_vdeg", "max_cdeg", "lds_messages", "threads", "device", "fixed_dc",
                "tail_at")
        return dict(zip(keys, list(out)))

    def set_tail(self, tail_at=-1):
        """First iteration of the tail launches (words still running after it
        are spread over several workgroups each; bit-identical).  -1: the
        default, 0: off (include/ldpc_bp.h lb_set_tail)."""
        _check(load_bp_library().lb_set_tail(self._context(), int(tail_at)))

    def Lxor(self, L1, L2, corrflag=1):
        """ldpc.py:932-935 (evaluated on the GPU)."""
        r = load_bp_library().Lxor(float(L1), float(L2), int(corrflag))
        if r != r and not (np.isnan(L1) or np.isnan(L2)):
            _check(-2)
        return r

    def Lxfb(self, L, corrflag=1):
        """ldpc.py:937-943: (aggregate LLR, extrinsic LLRs)."""
        L = np.array(L, dtype=float)
        r = load_bp_library().Lxfb(L.ctypes.data_as(_D), len(L), int(corrflag))
        if r != r and not np.isnan(L).any():
            _check(-2)
        return r, L

    def __del__(self):
        ctx = getattr(self, "_ctx", None)
        if ctx is not None and _lib is not None:
            try:
                _lib.lb_destroy(ctx)
            except Exception:
                pass
            self._ctx = None
