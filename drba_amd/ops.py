"""Tensor-level wrappers over the C ABI (include/drba_hip.h).

torch is used for device memory and the current HIP stream only: every function here
takes CUDA tensors, hands raw pointers to libdrba_hip.so on torch's current stream and
returns freshly allocated output tensors.  No arithmetic happens in torch.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from drba_amd import _lib
from drba_amd import tunecache as _tunecache

_MODES = {"sum": 0, "avg": 1, "linear": 2, "soft": 3}
_EPS = {None: 0, "addeps": 0, "zeroeps": 1, "clipeps": 2}


def default_device():
    if not torch.cuda.is_available():
        raise _lib.DrbaHipError("drba_amd needs an MI355X (no GPU visible and there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """The current HIP stream of the current device as a void*.  torch.cuda.current_stream() builds a Stream object through four
    Python frames (8.7 us per call, 23 000 calls per GMFSS_UNION step profiled: 0.2 of its 1.17 s of host time per 40 steps);
    the raw getter returns the handle."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, name="tensor"):
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise _lib.DrbaHipError(f"{name} is on {t.device}: drba_amd ops run on the GPU only (no CPU fallback)")
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


_ws_cache = {}
_ws_token = {}  # (device, stream) -> what the workspace's contents are good for (softsplat_many's sorted index), or absent


def _workspace(device, nfloats, keep_token=False):
    """Grow-only scratch per (device, stream): kernels on one stream are ordered, so reuse is safe.  Handing the buffer out
    invalidates whatever a previous user left in it (the splat index: `_ws_token`) unless that user asks for it back."""
    key = (device.index, _stream().value or 0)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nfloats:
        buf = torch.empty(max(int(nfloats), 1 << 20), dtype=torch.float32, device=device)
        _ws_cache[key] = buf
        _ws_token.pop(key, None)
    elif not keep_token:
        _ws_token.pop(key, None)
    return buf


_zero_ws_cache = {}


def _zero_workspace(device, nfloats):
    """Zero-initialised scratch per (device, stream) for the fused splats (drba_flow_reverse / drba_drm_rife_linear):
    their kernels return the accumulator (and the per-tile flags behind it) zeroed, so it is cleared once at allocation and never
    again.  The first MB is the kernels' reach map: plain scratch, written before it is read by every call (include/drba_hip.h)."""
    key = (device.index, _stream().value or 0)
    buf = _zero_ws_cache.get(key)
    if buf is None or buf.numel() < nfloats:
        buf = torch.zeros(max(int(nfloats), 1 << 20), dtype=torch.float32, device=device)
        _zero_ws_cache[key] = buf
    return buf


# Optional kernel trace (bench.py's roofline leg).  While TRACE is a list, the library times EVERY kernel it launches
# (drba_trace_begin: an event pair on each launch's own dispatch packet, so a record is the kernel's own execution time,
# as rocprofv3's kernel trace reports it -- an event recorded on the stream before/after a launch adds a barrier packet
# each side and reads ~10 us long).  The wrappers below that know their kernel's algorithmic work append
# (first trace index, [(work, unit, label), ...]) for the launches of the call they just made; bench.py joins these tags
# with the library's records (kernel name, grid, duration) after the timed region.
TRACE = None


def trace_begin():
    global TRACE
    _lib.check(_lib.load().drba_trace_begin(), "drba_trace_begin")
    TRACE = []


def trace_pause():
    """Stop recording (steps outside the instrumented ones); the records made so far stay readable."""
    _lib.check(_lib.load().drba_trace_end(), "drba_trace_end")


def trace_resume():
    _lib.check(_lib.load().drba_trace_resume(), "drba_trace_resume")


def trace_end():
    """-> [{"name", "grid", "ms", "work", "unit", "label"}] for every launch recorded, in launch order."""
    global TRACE
    lib = _lib.load()
    _lib.check(lib.drba_trace_end(), "drba_trace_end")
    tags, TRACE = TRACE or [], None
    recs = []
    name, grid, ms, t0, st = C.c_char_p(), (C.c_uint * 3)(), C.c_float(), C.c_float(), C.c_ulonglong()
    for i in range(lib.drba_trace_count()):
        _lib.check(lib.drba_trace_get(i, C.byref(name), grid, C.byref(ms)), "drba_trace_get")
        _lib.check(lib.drba_trace_get_start(i, C.byref(t0), C.byref(st)), "drba_trace_get_start")
        recs.append({"name": name.value.decode(), "grid": tuple(grid), "ms": float(ms.value), "work": None, "unit": None,
                     "label": None, "start_ms": float(t0.value), "stream": int(st.value)})
    for first, items in tags:
        for k, it in enumerate(items):
            if it is not None and first + k < len(recs):
                recs[first + k]["work"], recs[first + k]["unit"], recs[first + k]["label"] = it
    return recs


def _timed(kind, key, work, unit, launch):
    """Run `launch`; when tracing, tag its (single) kernel launch with its algorithmic work."""
    if TRACE is None:
        return launch()
    first = _lib.load().drba_trace_count()
    r = launch()
    TRACE.append((first, [(work, unit, f"{kind} {key}")]))
    return r


def _tag(first, items):
    if TRACE is not None:
        TRACE.append((first, items))


def _trace_pos():
    return _lib.load().drba_trace_count() if TRACE is not None else 0


# ----------------------------------------------------------------------------- overflow report of kernel family 4
# The two-term fp16 kernels overflow where fp32 does not (an activation of 65504 * 16 or more, an attention Q / V of 65504).  Every
# one of them folds the values it stores into a NaN test and sets its byte of a host-mapped status word (include/drba_hip.h,
# drba_status_word; ABI 8): no extra kernel, no synchronisation.  The model wrappers call status_init(device) when they are
# built and check_overflow(device) once per step; a set byte raises instead of handing inf / NaN frames on.  The read sees every
# kernel that has finished by then, a later one at the next step's read (sticky until cleared).
STATUS_GROUPS = ("conv_split (conv3x3 / deconv4x4)", "conv_dma (32-channel conv3x3)", "conv_ks (K-split conv3x3)", "linear_split",
                 "window_attention", "stage_conv16", "head_fused16")
_status_words = {}


def status_init(device=None):
    """Ask the library for the current (or given) device's status word; from then on its family-4 kernels report into it."""
    device = default_device() if device is None else torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx in _status_words:
        return
    ptr = C.c_void_p()
    with torch.cuda.device(idx):
        _lib.check(_lib.load().drba_status_word(C.byref(ptr)), "drba_status_word")
    _status_words[idx] = C.c_uint64.from_address(ptr.value)


def overflow_groups(device=None, clear=True):
    """Names of the kernel groups that have stored a non-finite value since the last clear (no synchronisation: kernels still
    in flight report at a later call)."""
    if not _status_words:  # nobody asked for a status word (status_init): nothing is reported
        return []
    device = None if device is None else torch.device(device)
    idx = device.index if (device is not None and device.index is not None) else torch.cuda.current_device()
    word = _status_words.get(idx)
    if word is None or word.value == 0:
        return []
    v = int(word.value)
    if clear:
        with torch.cuda.device(idx):
            _lib.load().drba_status_clear()
    return [STATUS_GROUPS[k] for k in range(len(STATUS_GROUPS)) if (v >> (8 * k)) & 0xff]


def check_overflow(device=None):
    bad = overflow_groups(device)
    if bad:
        raise _lib.DrbaHipError(
            "non-finite values out of the two-term fp16 kernels (family 4): " + ", ".join(bad) + " -- an activation beyond "
            "65504 * 16 (attention Q / V: 65504) overflowed fp16, or an input was already inf / NaN; the frames of this and the "
            "previous step are not to be trusted.  drba_amd.ops.set_precision({0, 1, 2, 3}) keeps every operand at 24 bits")


# ----------------------------------------------------------------------------- deterministic mode
# The library's switch (drba_set_deterministic) mirrored here, so that the per-call questions of this module cost no library call:
# DRBA_DETERMINISTIC=1 turns both on -- this one at import, the library's when it is loaded (_lib.load) --, which lets an unmodified
# bench.py time the mode.
_deterministic = os.environ.get("DRBA_DETERMINISTIC", "0") not in ("", "0")


def set_deterministic(on):
    """Bit-reproducible outputs (include/drba_hip.h, drba_set_deterministic): the splats sum in an order fixed
    by the data, and no timing decides a kernel configuration (_tune).  Process wide, off by default; switch it before the first
    frame -- kernel configurations are kept per mode.  -> the previous setting."""
    global _deterministic
    was = bool(_lib.load().drba_set_deterministic(1 if on else 0))
    _deterministic = bool(on)
    return was


def deterministic():
    return _deterministic


# ----------------------------------------------------------------------------- splat / warp / drm
def softsplat(tenIn, tenFlow, tenMetric, strMode, out=None, keep_quad=False):
    """`out` (not in the reference): a contiguous [N,C,H,W] destination, e.g. a channel slice of a concatenation buffer.
    keep_quad: see softsplat_many."""
    return softsplat_many([tenIn], tenFlow, tenMetric, strMode, None if out is None else [out], keep_quad=keep_quad)[0]


def _copy_of(t, attr, versioned=True):
    """The layout copy kept on tensor `t` as `attr`, or None.  versioned: kept as (copy, t._version), and a tensor written in
    place since has none (the library's own kernels write through raw pointers without bumping the version: see the callers)."""
    c = getattr(t, attr, None)
    if c is None or not versioned:
        return c
    return c[0] if c[1] == t._version else None


def _set_copy(t, attr, copy, versioned=True):
    setattr(t, attr, (copy, t._version) if versioned else copy)


def quad_interleaved(x):
    """[N,C,H,W] (C >= 16, C % 4 == 0) -> the [N][C/4][H*W][4] copy the feature gathers of the splat read, made once per tensor
    and kept on it (with the tensor's version: a tensor written in place since gets a new copy), or None for other channel
    counts.  The caller vouches that nothing writes the tensor through the library's raw pointers afterwards (those writes do not
    bump the version): GMFSS's cached FeatureNet pyramids are such tensors."""
    n, c, h, w = x.shape
    if c < 16 or c % 4:
        return None
    qt = _copy_of(x, "_drba_quad")
    if qt is None:
        qt = torch.empty((n, c // 4, h * w, 4), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().drba_quad_interleave(_p(x), _p(qt), n, c, h, w, _stream()), "drba_quad_interleave")
        _set_copy(x, "_drba_quad", qt)
    return qt


def softsplat_many(inputs, tenFlow, tenMetric, strMode, outs=None, reuse_index=False, keep_quad=False):
    """softsplat(x, tenFlow, tenMetric, strMode) for every x of `inputs` (same N, H, W; any channel counts): the sorted
    index of the (flow, metric, mode) is built once and every input is gathered through it (drba_softsplat_again) -- the
    count / scan / fill launches of the reference's one-call-per-tensor form are not repeated.  -> list of outputs.
    reuse_index=True: the caller vouches that the LAST splat on this stream used the same (flow, metric, mode, N, H, W) and
    channel counts no larger than before (the index is still in the stream's workspace): not even the first input rebuilds it.
    keep_quad=True: feature inputs (C >= 16, C % 4 == 0) are gathered from their quad-interleaved copies, made once per tensor
    and kept on it (quad_interleaved) instead of rewritten into the workspace by every call -- for inputs that outlive the call
    and are splatted again (GMFSS: every pyramid level of a frame, once per output frame of two consecutive steps)."""
    parts = strMode.split("-")
    main, sub = parts[0], (parts[1] if len(parts) > 1 else None)
    assert main in ("sum", "avg", "linear", "soft")
    if main in ("sum", "avg"):
        assert tenMetric is None
    if main in ("linear", "soft"):
        assert tenMetric is not None
    f = _f32(tenFlow, "tenFlow")
    m = None if tenMetric is None else _f32(tenMetric, "tenMetric")
    xs = [_f32(x, "tenIn") for x in inputs]
    n, _, h, w = xs[0].shape
    lib = _lib.load()
    ws = _workspace(f.device, max(lib.drba_softsplat_ws_floats(n, x.shape[1], h, w) for x in xs), keep_token=True)
    # what the index in `ws` was built from: the flow / metric tensors (storage + version), mode, geometry, the buffer and stream.
    # reuse_index=True is honoured only while that still holds -- another user of the workspace, a regrown buffer, an in-place
    # update of the flow or a call from another stream drops the token and the index is rebuilt (it used to be trusted blindly)
    # The token holds the flow / metric tensor OBJECTS (strong references: their storage cannot be freed and handed to another
    # tensor while the token lives -- an address + version pair alone could match a different flow that the caching allocator put at
    # the same address, the library's own kernels writing through raw pointers without bumping _version) and is not kept at all
    # when _f32 had to copy an argument (the copy is a temporary nobody can name again).
    wkey = (f.device.index, _stream().value or 0)
    copied = f is not tenFlow or (m is not None and m is not tenMetric)
    token = (f, f._version, m, None if m is None else m._version, strMode, n, h, w, ws.data_ptr())
    old = _ws_token.get(wkey)
    same = (old is not None and old[0] is token[0] and old[2] is token[2] and old[1] == token[1] and old[3] == token[3]
            and old[4:] == token[4:])
    if reuse_index and (copied or not same):
        reuse_index = False
    if copied:
        _ws_token.pop(wkey, None)
    else:
        _ws_token[wkey] = token
    res = []
    for k, x in enumerate(xs):
        assert x.shape[0] == n and tuple(x.shape[2:]) == (h, w), (tuple(x.shape), (n, h, w))
        c = x.shape[1]
        out = None if outs is None else outs[k]
        if out is None:
            out = torch.empty_like(x)
        elif tuple(out.shape) != tuple(x.shape) or not out.is_contiguous() or out.dtype != torch.float32:
            raise _lib.DrbaHipError("softsplat: out must be a contiguous float32 tensor of the input's shape")
        xq = quad_interleaved(inputs[k]) if keep_quad and inputs[k] is x else None  # (x is a private copy: nothing to keep it on)
        if xq is not None:
            if k == 0 and not reuse_index:
                _lib.check(lib.drba_softsplat_index(_p(f), _p(m), _p(ws), n, h, w, _MODES[main], _stream()), "drba_softsplat_index")
            _lib.check(lib.drba_softsplat_gather_quad(_p(xq), _p(out), _p(ws), n, c, h, w, _MODES[main], _EPS.get(sub, 0), _stream()),
                       "drba_softsplat_gather_quad")
        elif k == 0 and not reuse_index:
            _lib.check(lib.drba_softsplat(_p(x), _p(f), _p(m), _p(out), _p(ws), n, c, h, w, _MODES[main], _EPS.get(sub, 0),
                                          _stream()), "drba_softsplat")
        else:
            _lib.check(lib.drba_softsplat_again(_p(x), _p(out), _p(ws), n, c, h, w, _MODES[main], _EPS.get(sub, 0), _stream()),
                       "drba_softsplat_again")
        res.append(out)
    return res


def backwarp(x, flow, padding="border"):
    x, flow = _f32(x, "input"), _f32(flow, "flow")
    n, c, h, w = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().drba_backwarp(_p(x), _p(flow), _p(out), n, c, h, w, 0 if padding == "border" else 1,
                                         _stream()), "drba_backwarp")
    return out


def flow_distance(flow):
    flow = _f32(flow, "flow")
    n, _, h, w = flow.shape
    out = torch.empty((n, 1, h, w), dtype=torch.float32, device=flow.device)
    _lib.check(_lib.load().drba_flow_distance(_p(flow), _p(out), n, h, w, _stream()), "drba_flow_distance")
    return out


def flow_reverse(flow):
    flow = _f32(flow, "flow")
    n, _, h, w = flow.shape
    out = torch.empty_like(flow)
    ws = _zero_workspace(flow.device, _lib.load().drba_rife_splat_ws_floats(n, h, w, 2))
    first = _trace_pos()
    _lib.check(_lib.load().drba_flow_reverse(_p(flow), _p(out), _p(ws), n, h, w, _stream()), "drba_flow_reverse")
    _tag(first, [None, (16.0 * n * h * w, "byte", f"flow_reverse {(n, h, w)}")])  # long-flow prepass, then the tiled splat
    return out


def drm_rife_linear(flow_self, flow_other, t, eps=1e-4, t_dev=None):
    """`t_dev`: optional 1-element CUDA float tensor holding t (used instead of `t`; for graph replay)."""
    a, b = _f32(flow_self, "flow_self"), _f32(flow_other, "flow_other")
    n, _, h, w = a.shape
    out = torch.empty((n, 1, h, w), dtype=torch.float32, device=a.device)
    ws = _zero_workspace(a.device, _lib.load().drba_rife_splat_ws_floats(n, h, w, 1))
    first = _trace_pos()
    _lib.check(_lib.load().drba_drm_rife_linear(_p(a), _p(b), float(t), _p(t_dev), float(eps), _p(out), _p(ws), n, h,
                                                w, _stream()), "drba_drm_rife_linear")
    _tag(first, [None, (20.0 * n * h * w, "byte", f"drm_rife_linear {(n, h, w)}")])  # long-flow prepass, then the tiled splat
    return out


def drm_rife_linear_many(jobs, eps=1e-4):
    """drm_rife_linear(flow_self, flow_other, t, eps) for every (flow_self, flow_other, t) of `jobs` ([1,2,H,W] flows of one
    size) in ONE launch pair (drba_drm_rife_linear_batch; chunks of MAX_STAGE_ITEMS) -> list of [1,1,H,W] maps."""
    if not jobs:
        return []
    flows = [(_f32(a, "flow_self"), _f32(b, "flow_other"), float(t)) for a, b, t in jobs]
    _, _, h, w = flows[0][0].shape
    dev = flows[0][0].device
    res = []
    for c0 in range(0, len(flows), _lib.MAX_STAGE_ITEMS):
        chunk = flows[c0:c0 + _lib.MAX_STAGE_ITEMS]
        n = len(chunk)
        out = torch.empty((n, 1, h, w), dtype=torch.float32, device=dev)
        arr = (_lib.DrmJob * n)()
        for k, (a, b, t) in enumerate(chunk):
            if tuple(a.shape) != (1, 2, h, w) or tuple(b.shape) != (1, 2, h, w):
                raise _lib.DrbaHipError("drm_rife_linear_many: every flow must be [1,2,H,W] of one size")
            arr[k].flow_self, arr[k].flow_other, arr[k].t, arr[k].out = a.data_ptr(), b.data_ptr(), t, out[k].data_ptr()
        ws = _zero_workspace(dev, _lib.load().drba_rife_splat_ws_floats(n, h, w, 1))
        first = _trace_pos()
        _lib.check(_lib.load().drba_drm_rife_linear_batch(C.cast(arr, C.c_void_p), n, float(eps), _p(ws), h, w, _stream()),
                   "drba_drm_rife_linear_batch")
        _tag(first, [None, (20.0 * n * h * w, "byte", f"drm_rife_linear {(n, h, w)}")])
        res += [out[k:k + 1] for k in range(n)]
    return res


def drm_walk(t, precision=1e-3):
    """get_drm_t's scalar walk (reference drm.py:43-56) as the library makes it on the host -> (moves, n_moves): bit k of moves
    set = move k is the `_x < t` update, clear = the `_x > t` update.  None: longer than the 32-bit mask (DRBA_EUNSUPPORTED)."""
    moves, n = C.c_uint32(), C.c_int()
    rc = _lib.load().drba_drm_walk(float(t), float(precision), C.byref(moves), C.byref(n))
    if rc == _EUNSUPPORTED:
        return None
    _lib.check(rc, "drba_drm_walk")
    return moves.value, n.value


def _drm_rife_composed(flow_self, flow_other, t, eps, precision):
    """One direction of calc_drm_rife(linear=False) from the generic operators (what models/drm.py composes): the form for a
    walk the fused kernel's move mask cannot hold."""
    u = drm_retime(drm_ratio(flow_self, flow_other, eps)[1], t, precision)
    both = softsplat(torch.cat((u, affine(u, 0.0, 1.0)), 1), mul_map(flow_self, u), None, "avg")
    return fill_holes(both[:, 0:1].contiguous(), both[:, 1:2].contiguous(), u)


def drm_rife_nonlinear(flow_self, flow_other, t, eps=1e-4, precision=1e-3):
    """One direction of calc_drm_rife(linear=False) (reference drm.py:65-107) as one fused launch pair: the retimed ratio
    u = get_drm_t(d_other / (d_self + d_other), t), avg-splatted along flow_self * u, holes keeping u."""
    a, b = _f32(flow_self, "flow_self"), _f32(flow_other, "flow_other")
    n, _, h, w = a.shape
    out = torch.empty((n, 1, h, w), dtype=torch.float32, device=a.device)
    ws = _zero_workspace(a.device, _lib.load().drba_rife_splat_ws_floats(n, h, w, 1))
    first = _trace_pos()
    rc = _lib.load().drba_drm_rife_nonlinear(_p(a), _p(b), float(t), float(precision), float(eps), _p(out), _p(ws), n, h, w,
                                             _stream())
    if rc == _EUNSUPPORTED:  # a walk longer than the move mask (nothing was launched): the composition
        return _drm_rife_composed(a, b, t, eps, precision)
    _lib.check(rc, "drba_drm_rife_nonlinear")
    _tag(first, [None, (20.0 * n * h * w, "byte", f"drm_rife_nonlinear {(n, h, w)}")])  # long-flow prepass, then the tiled splat
    return out


def drm_rife_nonlinear_many(jobs, eps=1e-4, precision=1e-3):
    """drm_rife_nonlinear(flow_self, flow_other, t, eps, precision) for every (flow_self, flow_other, t) of `jobs` ([1,2,H,W] flows
    of one size) in ONE launch pair (drba_drm_rife_nonlinear_batch; chunks of MAX_STAGE_ITEMS) -> list of [1,1,H,W] maps."""
    if not jobs:
        return []
    flows = [(_f32(a, "flow_self"), _f32(b, "flow_other"), float(t)) for a, b, t in jobs]
    _, _, h, w = flows[0][0].shape
    dev = flows[0][0].device
    res = []
    for c0 in range(0, len(flows), _lib.MAX_STAGE_ITEMS):
        chunk = flows[c0:c0 + _lib.MAX_STAGE_ITEMS]
        n = len(chunk)
        out = torch.empty((n, 1, h, w), dtype=torch.float32, device=dev)
        arr = (_lib.DrmNonlinearJob * n)()
        for k, (a, b, t) in enumerate(chunk):
            if tuple(a.shape) != (1, 2, h, w) or tuple(b.shape) != (1, 2, h, w):
                raise _lib.DrbaHipError("drm_rife_nonlinear_many: every flow must be [1,2,H,W] of one size")
            arr[k].flow_self, arr[k].flow_other, arr[k].t, arr[k].out = a.data_ptr(), b.data_ptr(), t, out[k].data_ptr()
        ws = _zero_workspace(dev, _lib.load().drba_rife_splat_ws_floats(n, h, w, 1))
        first = _trace_pos()
        rc = _lib.load().drba_drm_rife_nonlinear_batch(C.cast(arr, C.c_void_p), n, float(precision), float(eps), _p(ws), h, w,
                                                       _stream())
        if rc == _EUNSUPPORTED:  # some walk of the chunk is longer than the move mask (nothing was launched)
            res += [drm_rife_nonlinear(a, b, t, eps, precision) for a, b, t in chunk]
            continue
        _lib.check(rc, "drba_drm_rife_nonlinear_batch")
        _tag(first, [None, (20.0 * n * h * w, "byte", f"drm_rife_nonlinear {(n, h, w)}")])
        res += [out[k:k + 1] for k in range(n)]
    return res


def drm_ratio(flow10, flow12, eps):
    a, b = _f32(flow10), _f32(flow12)
    n, _, h, w = a.shape
    r10 = torch.empty((n, 1, h, w), dtype=torch.float32, device=a.device)
    r12 = torch.empty_like(r10)
    _lib.check(_lib.load().drba_drm_ratio(_p(a), _p(b), float(eps), _p(r10), _p(r12), n, h, w, _stream()),
               "drba_drm_ratio")
    return r10, r12


def affine(a, mul, add):
    a = _f32(a)
    out = torch.empty_like(a)
    _lib.check(_lib.load().drba_affine(_p(a), float(mul), float(add), _p(out), a.numel(), _stream()), "drba_affine")
    return out


def mul_map(x, m):
    x, m = _f32(x), _f32(m)
    n, c, h, w = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().drba_mul_map(_p(x), _p(m), _p(out), n, c, h, w, _stream()), "drba_mul_map")
    return out


def fill_holes(aligned, cover, value):
    a, c, v = _f32(aligned), _f32(cover), _f32(value)
    out = torch.empty_like(a)
    _lib.check(_lib.load().drba_fill_holes(_p(a), _p(c), _p(v), _p(out), a.numel(), _stream()), "drba_fill_holes")
    return out


def drm_retime(drm, t, precision=1e-3):
    d = _f32(drm)
    out = torch.empty_like(d)
    _lib.check(_lib.load().drba_drm_retime(_p(d), _p(out), float(t), float(precision), d.numel(), _stream()),
               "drba_drm_retime")
    return out


# ----------------------------------------------------------------------------- resize / frames / scdet
def resize_bilinear(x, size):
    x = _f32(x)
    n, c, h, w = x.shape
    ho, wo = int(size[0]), int(size[1])
    out = torch.empty((n, c, ho, wo), dtype=torch.float32, device=x.device)
    sy, sx = _scales(False, (h, w), (ho, wo))
    nbytes = 4.0 * n * c * (min(h * w, 4 * ho * wo) + ho * wo)
    _lib.check(_timed("resize_bilinear", (n * c, h, w, ho, wo), nbytes, "byte", lambda: _lib.load().drba_resize_bilinear(
        _p(x), _p(out), n * c, h, w, ho, wo, sy, sx, _stream())), "drba_resize_bilinear")
    return out


def resize_bilinear_scale(x, size, src_scale):
    """F.interpolate(scale_factor=...) form: the coordinate multiplier is given explicitly (1/scale_factor)."""
    x = _f32(x)
    n, c, h, w = x.shape
    ho, wo = int(size[0]), int(size[1])
    out = torch.empty((n, c, ho, wo), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().drba_resize_bilinear(_p(x), _p(out), n * c, h, w, ho, wo, float(src_scale), float(src_scale),
                                                _stream()), "drba_resize_bilinear")
    return out


def _maxval(maxval):
    """The largest sample of a 16-bit frame: 65535 unless given (1023: 10-bit data); an integer in (255, 65535]."""
    if maxval is None:
        return 65535
    if int(maxval) != maxval or not 255 < int(maxval) <= 65535:
        raise ValueError(f"maxval of a 16-bit frame must be an integer with 255 < maxval <= 65535, got {maxval!r}")
    return int(maxval)


def _is_frame(t, dtype):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == 3 and t.shape[2] == 3


def _sample_kind(dtype, maxval):
    """What the frame paths of the two sample types differ in -> (bytes per sample, the tag of their trace kinds and library
    entries, the maxval argument the 16-bit entries take in front of the stream)."""
    if dtype == torch.uint16:
        return 2, "16", (float(_maxval(maxval)),)
    return 1, "", ()


def _hwc_to_f32nchw(img, dtype, maxval=None):
    if not _is_frame(img, dtype):
        raise _lib.DrbaHipError(f"expected a CUDA {str(dtype)[6:]} [H,W,3] tensor")
    size, _, mv = _sample_kind(dtype, maxval)
    img = img.contiguous()
    h, w = img.shape[:2]
    out = torch.empty((1, 3, h, w), dtype=torch.float32, device=img.device)
    name = f"u{8 * size}hwc_to_f32nchw"
    _lib.check(_timed(name, (h, w), (12.0 + 3.0 * size) * h * w, "byte", lambda: getattr(_lib.load(), "drba_" + name)(
        _p(img), _p(out), h, w, *mv, _stream())), "drba_" + name)
    return out


def _f32nchw_to_hwc(x, dtype, maxval=None):
    size, _, mv = _sample_kind(dtype, maxval)
    x = _f32(x)
    assert x.shape[0] == 1 and x.shape[1] == 3
    h, w = x.shape[2:]
    out = torch.empty((h, w, 3), dtype=dtype, device=x.device)
    name = f"f32nchw_to_u{8 * size}hwc"
    _lib.check(_timed(name, (h, w), (12.0 + 3.0 * size) * h * w, "byte", lambda: getattr(_lib.load(), "drba_" + name)(
        _p(x), _p(out), h, w, *mv, _stream())), "drba_" + name)
    return out


def u8hwc_to_f32nchw(img_u8):
    return _hwc_to_f32nchw(img_u8, torch.uint8)


def f32nchw_to_u8hwc(x):
    return _f32nchw_to_hwc(x, torch.uint8)


def u16hwc_to_f32nchw(img_u16, maxval=None):
    """u8hwc_to_f32nchw for a uint16 frame: / maxval."""
    return _hwc_to_f32nchw(img_u16, torch.uint16, maxval)


def f32nchw_to_u16hwc(x, maxval=None):
    """fp32 [1,3,H,W] -> uint16 [H,W,3]: x * maxval rounded to nearest even and saturated to [0, maxval], NaN -> 0."""
    return _f32nchw_to_hwc(x, torch.uint16, maxval)


FITS = ("resize", "pad")


def _fit(fit, way, frame, net):
    """`fit` of the four frame conversions -> whether it is "pad".  "resize" (the default, the reference's behaviour): the frame is
    resampled to the network size and back.  "pad": the frame sits at the top left of the network tensor, the bottom and right
    margins repeat its last row and column on the way in and are cropped away on the way out -- no interpolation in either
    direction, so the network tensor must be at least the frame."""
    if fit not in FITS:
        raise ValueError(f"fit must be one of {FITS}, got {fit!r}")
    if fit == "pad" and (net[0] < frame[0] or net[1] < frame[1]):
        raise ValueError(f"fit='pad' on the way {way}: the network tensor {tuple(net)} is smaller than the frame {tuple(frame)}")
    return fit == "pad"


def _scales(pad, src, dst):
    """the two coordinate multipliers of a resizing entry, ATen's static_cast<float>(in) / out; the pad / crop entries take none"""
    return () if pad else tuple(float(np.float32(s) / np.float32(d)) for s, d in zip(src, dst))


def _x4_like(out):
    """the [H,W,4] copy of the network input `out` that its kernel writes in the same pass: what the gathers read image taps from"""
    return torch.empty((out.shape[2], out.shape[3], 4), dtype=torch.float32, device=out.device) if IMG_X4 else None


def _with_x4(out, x4):
    if x4 is not None:
        _set_copy(out, "_drba_x4", x4)
    return out


def _plane_ptrs(planes, ny, nc):
    """the Y, U, V pointers of a packed planar tensor: `ny` samples of Y, then `nc` of U, then `nc` of V"""
    base, es = planes.data_ptr(), planes.element_size()
    return C.c_void_p(base), C.c_void_p(base + ny * es), C.c_void_p(base + (ny + nc) * es)


def _window(window, frame, sub=(1, 1), what="frame"):
    """`window` = (x, y, w, h) of the four frame conversions (--crop; ffmpeg's crop= names the same four numbers as w:h:x:y), checked
    against the frame (H, W): inside it, and for a planar frame -- sub = the layout's (horizontal, vertical) subsampling -- x, y
    multiples of it, w, h too unless the window reaches the frame's right / bottom edge (a chroma sample belongs to one side)."""
    try:
        x, y, w, h = (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"window must be (x, y, w, h), got {window!r}") from None
    fh, fw = int(frame[0]), int(frame[1])
    if x < 0 or y < 0 or w < 1 or h < 1 or x + w > fw or y + h > fh:
        raise ValueError(f"window {w}x{h} at ({x}, {y}) does not lie inside the {fw}x{fh} {what}")
    for name, at, ext, full, m in (("x", x, w, fw, sub[0]), ("y", y, h, fh, sub[1])):
        if at % m or (ext % m and at + ext != full):
            raise ValueError(f"window {w}x{h} at ({x}, {y}): {name} and the extent along it must be multiples of {m} for this chroma "
                             f"layout (the extent may be odd where the window reaches the {what}'s edge)")
    return x, y, w, h


def to_inp(img_u8, dst_size, maxval=None, fit="resize", window=None):
    """tools.to_inp on a device-resident frame: uint8 [H,W,3] -> fp32 [1,3,*dst_size] in [0,1], one kernel.  A uint16 [H,W,3]
    frame takes the 16-bit kernel: its samples are divided by `maxval` (65535 unless given; 255 < maxval <= 65535).
    fit="pad": replicate padding to `dst_size` instead of the resize (_fit).
    window=(x, y, w, h) (--crop): that rectangle of the frame is read in place, exactly as if it were the whole frame -- the values
    of to_inp on a contiguous copy of it, without the copy (the drba_to_inp*_win_x4 entries: a pointer and the frame's row pitch)."""
    if not (_is_frame(img_u8, torch.uint8) or _is_frame(img_u8, torch.uint16)):
        raise _lib.DrbaHipError("expected a CUDA uint8 or uint16 [H,W,3] tensor")
    size, tag, mv = _sample_kind(img_u8.dtype, maxval)
    img = img_u8.contiguous()
    h, w = img.shape[:2]
    ho, wo = int(dst_size[0]), int(dst_size[1])
    src, win, wtag = _p(img), (), ""  # no window: the entries the call always made
    if window is not None:
        x0, y0, ww, wh = _window(window, (h, w))
        src, win, wtag = C.c_void_p(img.data_ptr() + (y0 * w + x0) * 3 * size), (3 * w,), "_win"  # its first sample, the frame's pitch
        h, w = wh, ww
    out = torch.empty((1, 3, ho, wo), dtype=torch.float32, device=img.device)
    x4 = _x4_like(out)
    pad = _fit(fit, "in", (h, w), (ho, wo))
    scales = _scales(pad, (h, w), (ho, wo))
    entry = f"drba_to_inp{tag}_pad{wtag}_x4" if pad else f"drba_to_inp{tag}{wtag}_x4"
    _lib.check(_timed("to_inp" + tag + ("_pad" if pad else ""), (h, w, ho, wo),
                      3.0 * size * min(h * w, 4 * ho * wo) + (28.0 if IMG_X4 else 12.0) * ho * wo, "byte",
                      lambda: getattr(_lib.load(), entry)(src, *win, _p(out), _p(x4), h, w, ho, wo, *scales, *mv, _stream())), entry)
    return _with_x4(out, x4)


def to_out(x, src_size, rgb=False, depth=8, maxval=None, fit="resize", window=None):
    """tools.to_out without the D2H copy: fp32 [1,3,h,w] -> uint8 [*src_size,3] on the device, one kernel
    (resize + *255. truncation; rgb=True also flips BGR -> RGB for the encoder pipe).
    depth=16: a torch.uint16 [*src_size,3] frame instead -- resize, * maxval (65535 unless given), rounded to nearest even and
    saturated to [0, maxval], NaN -> 0: the 8-bit path keeps the reference's truncation because its bytes must equal the
    reference's, a 16-bit frame has no reference to equal.
    fit="pad": the top-left `src_size` window of x is quantised as it stands instead of the resize (_fit).
    window=(x, y, w, h) (--crop): the frame is still [*src_size,3], but x is converted to the w x h rectangle at (x, y) of it -- the
    samples of to_out(x, (h, w)) -- and everything outside the rectangle is black, 0, 0, 0: what this conversion writes for an
    all-zero tensor (one fill, then the drba_to_out*_win entries: a pointer and the frame's row pitch)."""
    if depth not in (8, 16):
        raise ValueError(f"depth must be 8 or 16, got {depth!r}")
    if depth == 8 and maxval is not None:
        raise ValueError("maxval belongs to 16-bit frames (depth=16)")
    x = _f32(x)
    assert x.shape[0] == 1 and x.shape[1] == 3
    h, w = x.shape[2:]
    ho, wo = int(src_size[0]), int(src_size[1])
    dtype = torch.uint16 if depth == 16 else torch.uint8
    size, tag, mv = _sample_kind(dtype, maxval)
    if window is None:
        out = torch.empty((ho, wo, 3), dtype=dtype, device=x.device)
        dst, win, wtag = _p(out), (), ""  # the entries the call always made
    else:
        x0, y0, ww, wh = _window(window, (ho, wo))
        out = torch.zeros((ho, wo, 3), dtype=dtype, device=x.device)
        dst, win, wtag = C.c_void_p(out.data_ptr() + (y0 * wo + x0) * 3 * size), (3 * wo,), "_win"  # its first sample, the frame's pitch
        ho, wo = wh, ww
    pad = _fit(fit, "out", (ho, wo), (h, w))
    scales = _scales(pad, (h, w), (ho, wo))
    entry = "drba_to_out" + tag + ("_crop" if pad else "") + wtag
    _lib.check(_timed("to_out" + tag + ("_crop" if pad else ""), (h, w, ho, wo), 12.0 * min(h * w, 4 * ho * wo) + 3.0 * size * ho * wo, "byte",
                      lambda: getattr(_lib.load(), entry)(_p(x), dst, *win, h, w, ho, wo, *scales, 1 if rgb else 0, *mv, _stream())), entry)
    return out


YUV_MATRICES = {"bt709": 0, "bt601": 1}


def _yuv_args(matrix, depth, maxval):
    """-> (matrix id, sample dtype, tag of the library entries, the maxval argument).  depth 8: bytes; 16: uint16 samples in
    [0, maxval], 1023 (10-bit, what YUV4MPEG2 carries) unless given."""
    if matrix not in YUV_MATRICES:
        raise ValueError(f"matrix must be one of {sorted(YUV_MATRICES)}, got {matrix!r}")
    if depth not in (8, 16):
        raise ValueError(f"depth must be 8 or 16, got {depth!r}")
    if depth == 8:
        if maxval not in (None, 255):
            raise ValueError("maxval belongs to 16-bit samples (depth=16)")
        return YUV_MATRICES[matrix], torch.uint8, "", ()
    return YUV_MATRICES[matrix], torch.uint16, "16", (float(_maxval(1023 if maxval is None else maxval)),)


def yuv420_layout(size):
    """(H, W) -> (samples of Y, of U (= of V), Hc, Wc) of a packed planar 4:2:0 frame: Y, then U, then V, rows without padding"""
    h, w = int(size[0]), int(size[1])
    hc, wc = (h + 1) // 2, (w + 1) // 2
    return h * w, hc * wc, hc, wc


YUV_LAYOUTS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}  # name -> (horizontal, vertical) subsampling factor of U and V


YUV_SAMPLES_PER_PIXEL = {"420": 1.5, "422": 2.0, "444": 3.0}  # the byte model of the conversions (_timed)


def yuv_layout(size, layout="420"):
    """yuv420_layout for any of YUV_LAYOUTS: U and V are [ceil(H / sy)][ceil(W / sx)]"""
    if layout not in YUV_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(YUV_LAYOUTS)}, got {layout!r}")
    sx, sy = YUV_LAYOUTS[layout]
    h, w = int(size[0]), int(size[1])
    hc, wc = (h + sy - 1) // sy, (w + sx - 1) // sx
    return h * w, hc * wc, hc, wc


def _yuv_name(layout):
    return "4:" + ":".join(layout[1:])


def _plane_window(base, es, frame, layout, window, what):
    """A window of a packed planar frame at address `base` -> ((Y, U, V) pointers of its first samples, (h, w) of the window): pointer
    arithmetic only, the strides stay the frame's (W and the chroma width).  The chroma offset is the window's origin divided by the
    layout's subsampling, which is why _window asks for multiples of it."""
    sx, sy = YUV_LAYOUTS[layout]
    x0, y0, ww, wh = _window(window, frame, (sx, sy), what)
    ny, nc, _, wc = yuv_layout(frame, layout)
    off_y, off_c = y0 * int(frame[1]) + x0, (y0 // sy) * wc + x0 // sx
    return (C.c_void_p(base + off_y * es), C.c_void_p(base + (ny + off_c) * es), C.c_void_p(base + (ny + nc + off_c) * es)), (wh, ww)


_BLACK_YUV = {}  # (device, dtype, size, layout, matrix, range, maxval) -> the planar frame to_out_yuv writes for an all-zero tensor
_BLACK_YUV_KEPT = 4  # formats kept: a run has one; each is one frame of device memory (3 MB at 1080p 4:2:0) held until it is pushed out


def _black_yuv(device, size, matrix, full_range, depth, maxval, layout):
    """The planar frame of `size` that to_out_yuv writes for an all-zero network tensor -- the range's black code, mid-grey chroma --,
    made once per format by that very conversion (one stream synchronisation, on that first call only) and kept in device memory for
    the life of the process, the last _BLACK_YUV_KEPT formats: a windowed frame starts as a copy of it."""
    key = (str(device), depth, tuple(size), layout, matrix, bool(full_range), maxval)
    t = _BLACK_YUV.get(key)
    if t is None:
        if len(_BLACK_YUV) >= _BLACK_YUV_KEPT:
            _BLACK_YUV.pop(next(iter(_BLACK_YUV)))  # the oldest
        t = to_out_yuv(torch.zeros((1, 3, 8, 8), dtype=torch.float32, device=device), size, matrix=matrix, full_range=full_range,
                       depth=depth, maxval=maxval, layout=layout)
        torch.cuda.current_stream(t.device).synchronize()  # made on this stream, copied from on whichever stream asks later
        _BLACK_YUV[key] = t
    return t


def to_inp_yuv(planes, size, dst_size, matrix="bt709", full_range=False, maxval=None, fit="resize", layout="420", window=None):
    """to_inp for a planar YCbCr frame on the device: `planes` is one contiguous 1-D tensor holding Y [H,W], then U, then V
    ([ceil(H/2),ceil(W/2)] for layout "420", [H,ceil(W/2)] for "422", [H,W] for "444") of a frame of `size` = (H, W) -- uint8
    samples, or uint16 ones in [0, maxval] (1023 unless given) -- -> fp32 [1,3,*dst_size] in [0,1], BGR channel order, one kernel:
    chroma interpolation (along the subsampled axes only), colour conversion and the resize (include/drba_hip.h, ABI 14 and 16).
    The [H,W,4] copy is written in the same pass, as in to_inp.
    fit="pad": the converted frame is replicate-padded to `dst_size` instead of resized (_fit); a margin pixel is the converted
    pixel of the clamped source coordinate.
    window=(x, y, w, h) (--crop): that rectangle of the frame is converted in place as if it were the whole frame (plane pointers
    moved, strides kept: _plane_window); x, y -- and w, h unless the window reaches the right / bottom edge -- are multiples of the
    layout's subsampling."""
    if not (torch.is_tensor(planes) and planes.is_cuda and planes.dim() == 1 and planes.dtype in (torch.uint8, torch.uint16)):
        raise _lib.DrbaHipError("expected a CUDA uint8 or uint16 1-D tensor of packed Y, U, V planes")
    mid, dtype, tag, mv = _yuv_args(matrix, 8 if planes.dtype == torch.uint8 else 16, maxval)
    h, w = int(size[0]), int(size[1])
    ny, nc, _, wc = yuv_layout((h, w), layout)
    planes = planes.contiguous()
    if planes.numel() != ny + 2 * nc:
        raise _lib.DrbaHipError(f"a {w}x{h} {_yuv_name(layout)} frame is {ny + 2 * nc} samples, got {planes.numel()}")
    ho, wo = int(dst_size[0]), int(dst_size[1])
    out = torch.empty((1, 3, ho, wo), dtype=torch.float32, device=planes.device)
    x4 = _x4_like(out)
    es, (y, u, v) = planes.element_size(), _plane_ptrs(planes, ny, nc)
    fw = w  # the luma stride is the frame's width, whatever is read of it
    if window is not None:
        (y, u, v), (h, w) = _plane_window(planes.data_ptr(), es, (h, w), layout, window, "frame")
    pad = _fit(fit, "in", (h, w), (ho, wo))
    scales = _scales(pad, (h, w), (ho, wo))
    # 4:2:0 keeps its own entries (and names in the trace and the profiles); the other layouts say which they are
    fmt, lay = ("yuv420", ()) if layout == "420" else ("yuv", (int(layout),))
    entry = f"drba_to_inp{tag}_{fmt}_pad_x4" if pad else f"drba_to_inp{tag}_{fmt}_x4"
    name = "to_inp_yuv" + ("" if layout == "420" else layout) + tag + ("_pad" if pad else "")
    _lib.check(_timed(name, (h, w, ho, wo),
                      YUV_SAMPLES_PER_PIXEL[layout] * es * min(h * w, 4 * ho * wo) + (28.0 if IMG_X4 else 12.0) * ho * wo, "byte",
                      lambda: getattr(_lib.load(), entry)(y, u, v, fw, wc, _p(out), _p(x4), h, w, ho, wo, *scales, mid, 1 if full_range else 0,
                                                          *lay, *mv, _stream())), entry)
    return _with_x4(out, x4)


def to_out_yuv(x, src_size, matrix="bt709", full_range=False, depth=8, maxval=None, fit="resize", layout="420", window=None):
    """to_out to a planar YCbCr frame on the device: fp32 [1,3,h,w] (BGR) -> ONE contiguous 1-D tensor holding Y [*src_size],
    then U, then V (their sizes by `layout`, as in to_inp_yuv), uint8 (depth 8) or uint16 scaled to `maxval` (depth 16; 1023 unless
    given): resize, clamp, colour conversion, the chroma mean (2 x 2 for "420", the horizontal pair for "422", none for "444"),
    round to nearest even, in one kernel.  One D2H copy and one write per frame.
    fit="pad": the top-left `src_size` window of x is converted as it stands instead of the resize (_fit); the chroma mean never
    reads the margin.
    window=(x, y, w, h) (--crop): the frame is still that of `src_size`, but x is converted to the w x h rectangle at (x, y) of it --
    the samples of to_out_yuv(x, (h, w)) -- and everything outside is black: the samples this conversion writes for an all-zero
    tensor (_black_yuv, copied per frame).  x, y, w, h as in to_inp_yuv."""
    mid, dtype, tag, mv = _yuv_args(matrix, depth, maxval)
    x = _f32(x)
    assert x.shape[0] == 1 and x.shape[1] == 3
    h, w = x.shape[2:]
    ho, wo = int(src_size[0]), int(src_size[1])
    ny, nc, _, wc = yuv_layout((ho, wo), layout)
    fw = wo  # the luma stride is the frame's width, whatever is written of it
    if window is None:
        pad = _fit(fit, "out", (ho, wo), (h, w))
        scales = _scales(pad, (h, w), (ho, wo))
        out = torch.empty(ny + 2 * nc, dtype=dtype, device=x.device)
        es, (y, u, v) = out.element_size(), _plane_ptrs(out, ny, nc)
    else:
        out = _black_yuv(x.device, (ho, wo), matrix, full_range, depth, maxval, layout).clone()
        es = out.element_size()
        (y, u, v), (ho, wo) = _plane_window(out.data_ptr(), es, (ho, wo), layout, window, "frame")
        pad = _fit(fit, "out", (ho, wo), (h, w))
        scales = _scales(pad, (h, w), (ho, wo))
    fmt, lay = ("yuv420", ()) if layout == "420" else ("yuv", (int(layout),))
    entry = f"drba_to_out{tag}_{fmt}" + ("_crop" if pad else "")
    name = "to_out_yuv" + ("" if layout == "420" else layout) + tag + ("_crop" if pad else "")
    _lib.check(_timed(name, (h, w, ho, wo), 12.0 * min(h * w, 4 * ho * wo) + YUV_SAMPLES_PER_PIXEL[layout] * es * ho * wo, "byte",
                      lambda: getattr(_lib.load(), entry)(_p(x), y, u, v, fw, wc, h, w, ho, wo, *scales, mid, 1 if full_range else 0, *lay,
                                                          *mv, _stream())), entry)
    return out


def _ssim_thumb32_enqueue(x1, x2):
    """The two thumbnails and the SSIM kernel on the current stream -> the device tensor [1] the value lands in."""
    a, b = resize_bilinear(x1, (32, 32)), resize_bilinear(x2, (32, 32))
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().drba_ssim3d_32(_p(a), _p(b), _p(out), _stream()), "drba_ssim3d_32")
    return out


def ssim_thumb32(x1, x2):
    """check_scene's metric: 32x32 bilinear thumbnails -> 3-D gaussian SSIM.  Returns a Python float
    (one D2H read: the driver branches on it, exactly like the reference's `if check_scene(...)`)."""
    return float(_ssim_thumb32_enqueue(x1, x2).item())


def ssim_thumb32_async(x1, x2):
    """The same metric without waiting for it: -> (pinned host tensor [1], event).  The driver asks for the test of a frame
    pair when the second frame is READ -- three iterations before it branches on it -- and reads the value after
    event.synchronize(): by then the two small kernels have long run, and the host no longer drains the whole queue of
    synthesis kernels once per source frame to learn one float."""
    out = _ssim_thumb32_enqueue(x1, x2)
    host = torch.empty(1, dtype=torch.float32, pin_memory=True)
    host.copy_(out, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(out.device))
    return host, ev


def _edge_max_enqueue(frame, group=None):
    """drba_edge_max_u8 / _u16 on the current stream -> (one device int32 tensor holding row_max then col_max, the number of rows)."""
    if not (torch.is_tensor(frame) and frame.is_cuda and frame.dtype in (torch.uint8, torch.uint16) and frame.dim() in (2, 3)):
        raise _lib.DrbaHipError("edge_max takes a CUDA uint8 or uint16 tensor: a packed frame [H,W,c] or a plane [rows,cols]")
    if frame.dim() == 3:  # a packed frame, seen as H x cW samples
        rows, cols, pitch = int(frame.shape[0]), int(frame.shape[1] * frame.shape[2]), int(frame.stride(0))
        ok = frame.stride(2) == 1 and frame.stride(1) == frame.shape[2]
        group = int(frame.shape[2]) if group is None else int(group)
    else:
        rows, cols, pitch = int(frame.shape[0]), int(frame.shape[1]), int(frame.stride(0))
        ok = frame.stride(1) == 1
        group = 1 if group is None else int(group)
    if rows == 1:
        pitch = max(pitch, cols)  # (the stride of an axis of size 1 is arbitrary)
    if not ok or rows < 1 or cols < 1 or pitch < cols:
        raise _lib.DrbaHipError(f"edge_max reads rows of contiguous samples, got shape {tuple(frame.shape)} strides {tuple(frame.stride())}")
    if group < 1 or cols % group:
        raise ValueError(f"group must divide the {cols} samples of a row, got {group}")
    out = torch.empty(rows + cols // group, dtype=torch.int32, device=frame.device)
    entry = "drba_edge_max_u8" if frame.dtype == torch.uint8 else "drba_edge_max_u16"
    first = _trace_pos()
    _lib.check(getattr(_lib.load(), entry)(_p(frame), rows, cols, pitch, group, _p(out), C.c_void_p(out.data_ptr() + 4 * rows), _stream()),
               entry)
    _tag(first, [None, (float(frame.element_size()) * rows * cols, "byte", f"edge_max {(rows, cols, group)}")])  # the zeroing, then the pass
    return out, rows


def edge_max(frame, group=None):
    """The active-picture statistic of --crop (include/drba_hip.h: drba_edge_max_u8 / _u16) -> (row_max [rows], col_max [cols / group]),
    two device int32 tensors: the largest sample of every row, and of every pixel column over the rows and the `group` samples of a
    pixel.  `frame`: a packed uint8 / uint16 frame [H,W,3] (group 3 unless given: H x 3W samples) or a plane [rows,cols] (group 1),
    whose rows may be a view with a pitch.  drba_amd.crop.box_of turns the two arrays into the picture's box."""
    out, rows = _edge_max_enqueue(frame, group)
    return out[:rows], out[rows:]


def edge_max_async(frame, group=None):
    """The same without waiting for it: -> (pinned host int32 tensor holding row_max then col_max, event, rows), as dup_stats_async;
    the arrays are read after event.synchronize()."""
    out, rows = _edge_max_enqueue(frame, group)
    host = torch.empty(out.numel(), dtype=torch.int32, pin_memory=True)
    host.copy_(out, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(out.device))
    return host, ev, rows


def _dup_stats_enqueue(x1, x2, lo):
    """drba_dup_stats_f32 on the current stream -> the device tensor [3] (int32 words: max_block's float bits, n_above, n_blocks)."""
    a, b = _f32(x1, "x1"), _f32(x2, "x2")
    if a.dim() != 4 or a.shape[0] != 1 or a.shape != b.shape:
        raise ValueError(f"dup_stats takes two [1, c, h, w] tensors of one shape, got {tuple(x1.shape)} and {tuple(x2.shape)}")
    c, h, w = (int(v) for v in a.shape[1:])
    lib = _lib.load()
    out = torch.empty(3, dtype=torch.int32, device=a.device)
    ws = torch.empty(max(int(lib.drba_dup_stats_ws_floats(c, h, w)), 1), dtype=torch.float32, device=a.device)
    first = _trace_pos()
    _lib.check(lib.drba_dup_stats_f32(_p(a), _p(b), c, h, w, float(lo), _p(out), _p(ws), _stream()), "drba_dup_stats_f32")
    _tag(first, [(8.0 * c * h * w, "byte", f"dup_stats {(c, h, w)}"), None])  # the streaming pass, then the fold of its partials
    return out


def dup_stats_decode(host):
    """The three words drba_dup_stats_f32 wrote, on the host -> (max_block, n_above, n_blocks) as Python numbers."""
    return float(host[:1].view(torch.float32).item()), int(host[1].item()), int(host[2].item())


def dup_stats(x1, x2, lo):
    """The duplicate-frame statistic of two network inputs [1, c, h, w] (include/drba_hip.h: drba_dup_stats_f32): the largest mean of
    |x1 - x2| over an 8 x 8 block, the number of blocks whose mean is > lo, the number of blocks.  One D2H read."""
    return dup_stats_decode(_dup_stats_enqueue(x1, x2, lo).cpu())


def dup_stats_async(x1, x2, lo):
    """The same without waiting for it: -> (pinned host tensor [3] int32, event), as ssim_thumb32_async.  The words are read
    (dup_stats_decode) after event.synchronize() -- that test's own event: the caller's stream is never drained."""
    out = _dup_stats_enqueue(x1, x2, lo)
    host = torch.empty(3, dtype=torch.int32, pin_memory=True)
    host.copy_(out, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(out.device))
    return host, ev


# ----------------------------------------------------------------------------- convolutions
# Kernel-configuration choice.  The library's cost model gives a default; with AUTOTUNE on (default) the
# first call for a new layer shape times every configuration built for that stride once on the device
# and keeps the fastest ("measure, don't guess").  Results are shared by all layers of the same shape.
AUTOTUNE = True
# kernel families the autotuner may choose from (drba_conv3x3_cfg_family: 0 fp32 MFMA, 1 split-bf16 register staging, 2 LDS-DMA
# 32-channel, 3 K-split, 4 the two-term fp16 split: 22-bit operands, half the matrix-core work, errors against fp64 at
# the same fp32-accumulation floor as the others); A/B runs narrow it (tools/ab_bench.py --conv-families), and
# CONV_FAMILIES = {0, 1, 2, 3} before the first call keeps every operand at 24 bits
CONV_FAMILIES = {0, 1, 2, 3, 4}
_tuned = {}
_tuned_det = {}  # the choices of the deterministic mode (shape-only or stored; never timed here): kept apart from the timed winners


def _tuned_table():
    return _tuned_det if deterministic() else _tuned


def set_precision(families):
    """The kernel families every tuner / kernel switch of this module may use from now on ({0, 1, 2, 3}: 24-bit operands everywhere;
    + 4: the two-term fp16 split).  May be called at any time: winners are cached per (shape, families) and the switches that
    follow CONV_FAMILIES (encoder, linears, window attention, fused stage) read it at every call."""
    global CONV_FAMILIES
    CONV_FAMILIES = {int(f) for f in families}


def two_term_ok(w):
    """Can kernel family 4 hold these weights?  It keeps a weight as fp16(w) + 2^-11 fp16(...) without a pre-scale: |w| >= 65504 (or
    a non-finite one) is beyond it -- the library's *_pack entry points refuse such a tensor (DRBA_EUNSUPPORTED, ABI 8) -- and the
    layer is run by a 24-bit family instead (its own tuner entry: _families)."""
    w = w.detach().float()
    return bool(torch.isfinite(w).all()) and (w.numel() == 0 or float(w.abs().max()) < 65504.0)


def _two_term(forced, weights_ok=True):
    """Kernel family 4 (two fp16 terms per operand) or a 24-bit form, wherever a kernel exists in both: a forced value (the
    *_TWO_TERM switches: tests, A/B) wins, otherwise family 4 must be allowed (read at every call: set_precision) and able to hold
    the weights (two_term_ok)."""
    return bool(forced) if forced is not None else (4 in CONV_FAMILIES and bool(weights_ok))


def _families(layer_ok=True):
    """The kernel families a layer may use: CONV_FAMILIES, without family 4 for a layer whose weights it cannot hold."""
    return CONV_FAMILIES if layer_ok else CONV_FAMILIES - {4}


def _candidates(lib, kind, stride, families, cin, cout):
    """The configuration ids a tuner may time for a cin -> cout layer of `kind` ("conv3x3" / "deconv4x4"): built for `stride` (None
    for the transposed convolution, whose ids carry none), of one of `families`, and able to run the layer (packed_floats 0: the
    configuration cannot)."""
    num, family, packed = (getattr(lib, f"drba_{kind}_{what}") for what in ("num_cfgs", "cfg_family", "packed_floats"))
    return [c for c in range(num()) if (stride is None or lib.drba_conv3x3_cfg_stride(c) == stride)
            and family(c) in families and packed(cin, cout, c) > 0]


def _tuned_get(shape_key, families=None):
    return _tuned_table().get((shape_key, tuple(sorted(CONV_FAMILIES if families is None else families))))


class NoKernelConfig(_lib.DrbaHipError):
    """No kernel configuration accepts a shape (every candidate's warm launch refused it)."""


_no_config = set()  # keys of _tuned's kind for which every candidate refused: not asked again in this process
TUNE_IGNORE_HITS = False  # drba_amd.tune --retune: stored winners are not read, every shape met is tuned afresh and its entry replaced
_TUNE_STAT_KEYS = ("full_tunes", "timing_passes", "cache_hits", "negative_hits", "rejected", "stored")
_tune_stats = dict.fromkeys(_TUNE_STAT_KEYS, 0)


def tune_stats():
    """What the autotuner did in this process so far: shapes tuned in full, timing passes (one device synchronisation each),
    winners taken from the store (drba_amd.tunecache; `negative_hits`: stored "no configuration accepts"), stored entries that were
    rejected, entries written."""
    return dict(_tune_stats)


_EUNSUPPORTED = -2  # DRBA_EUNSUPPORTED (include/drba_hip.h): the shape is outside what the configuration was built for


def _tune(shape_key, candidates, run, reps=3, families=None, persist=False, device=None, pick=None):
    """persist: the winner is looked up in / written to the store of drba_amd.tunecache when DRBA_TUNE_CACHE turns it on (the
    three convolution wrappers below pass it, with the index of the device the layer runs on; keys of any other caller are never
    stored).
    Deterministic mode (set_deterministic): no timing decides anything.  A stored winner is taken as always (that path never timed);
    otherwise the choice follows from the shape alone -- `pick()`, the library's *_pick_cfg answer, when it is a candidate and its
    warm launch accepts the shape, else the first candidate that does -- with no timing pass, no synchronisation and nothing
    written to the store: two runs agree given the same build, device model, store contents and command."""
    # a winner of one family set is not offered to another
    fams = tuple(sorted(CONV_FAMILIES if families is None else families))
    kind_key, shape_key = shape_key, (shape_key, fams)
    det = deterministic()
    table = _tuned_det if det else _tuned
    if shape_key in table:
        return table[shape_key]
    if shape_key in _no_config:
        raise NoKernelConfig(f"no kernel configuration accepts {shape_key}")
    # (with the library's debug range check armed a launch can return DRBA_EUNSUPPORTED for what is in the DATA: nothing such a
    # process learns is a property of the shape, so it neither reads nor writes the store)
    store = _tunecache.active(device) if persist and os.environ.get("DRBA_CHECK_RANGE", "0") in ("", "0") else None
    if store is not None and not TUNE_IGNORE_HITS:
        hit = store.get(kind_key, fams)
        if hit is not None:
            if hit.get("none"):
                _tune_stats["negative_hits"] += 1
                _no_config.add(shape_key)
                raise NoKernelConfig(f"no kernel configuration accepts {shape_key}")
            # an id from the file is launched only if this process offers it for the layer itself; its one warm launch must succeed
            code = run(hit["cfg"]) if hit["cfg"] in candidates else _EUNSUPPORTED
            if code == 0:
                _tune_stats["cache_hits"] += 1
                table[shape_key] = hit["cfg"]
                return hit["cfg"]
            if code != _EUNSUPPORTED:  # a launch failure / bad argument says nothing about the entry: not rejected, not re-tuned over
                raise _lib.DrbaHipError(f"warm launch of the stored configuration {hit['cfg']} for {shape_key} failed ({code})")
            _tune_stats["rejected"] += 1

    if det:
        first = pick() if callable(pick) else pick
        for cfg in ([first] if first in candidates else []) + [c for c in candidates if c != first]:
            code = run(cfg)  # the one warm launch: does the configuration accept the shape?
            if code == 0:
                table[shape_key] = cfg
                return cfg
            if code != _EUNSUPPORTED:
                raise _lib.DrbaHipError(f"warm launch of configuration {cfg} for {shape_key} failed ({code})")
        _no_config.add(shape_key)  # (a property of the shape; remembered in the process, not in the store)
        raise NoKernelConfig(f"no kernel configuration accepts {shape_key}")

    def timed(cfg):
        # the candidates are timed on an otherwise idle device: the first call for a shape usually comes from inside the
        # three-stream pipeline, and a candidate timed beside another stream's kernels loses to one that was not (round 4: a
        # 590 us stride-2 tile picked over a 321 us one for the largest conv0 layer, -1.5 % on the step)
        torch.cuda.synchronize()
        _tune_stats["timing_passes"] += 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run(cfg)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    _tune_stats["full_tunes"] += 1
    codes = {cfg: run(cfg) for cfg in candidates}  # warm: packs weights, faults pages; a configuration that refuses the shape is not a candidate
    ok = [cfg for cfg in candidates if codes[cfg] == 0]
    if not ok:
        if any(c != _EUNSUPPORTED for c in codes.values()):
            # a launch failure (DRBA_ELAUNCH, a sticky earlier error) or a bad argument is not a property of the shape: it is
            # reported as it always was and remembered nowhere, neither in the process nor in the store
            raise _lib.DrbaHipError(f"no kernel configuration accepts {shape_key}: the warm launches failed with {sorted(set(codes.values()))}")
        _no_config.add(shape_key)  # no candidate, or every one answered DRBA_EUNSUPPORTED
        if store is not None and store.put(kind_key, fams, None):
            _tune_stats["stored"] += 1
        raise NoKernelConfig(f"no kernel configuration accepts {shape_key}")
    first = {cfg: timed(cfg) for cfg in ok}
    # Every candidate is read twice (the second pass in reverse order) and its smaller reading counts.  Round 6: 38 convolution
    # configurations, several within a few percent of each other on most layers, and one reading in a few hundred carries a one-off
    # delay of milliseconds (tools/exp/cfg37_probe.py: the same launch 94 us and 4111 us) -- a single pass picked a 4 % slower
    # tile for a layer in some runs and could lose the true best to such a reading (the 24-bit headline leg read 880 once, 950-976
    # otherwise).  ~20 ms per layer shape, once per process (once per machine and build with the store on).
    second = {cfg: timed(cfg) for cfg in reversed(ok)} if len(ok) > 1 else first
    reading = {c: min(first[c], second[c]) for c in ok}
    best = min(ok, key=lambda c: reading[c])
    _tuned[shape_key] = best
    if store is not None:
        us = sorted(reading[c] for c in ok if c != best)
        if store.put(kind_key, fams, best, reading[best] * 1e3 / reps, us[0] * 1e3 / reps if us else None):
            _tune_stats["stored"] += 1
    return best


def conv_state_reset():
    """drba_conv_state_reset on the current stream: the family-2 convolution's per-stream work counters back to their initial
    state (first thing inside a stream capture, and before eager launches that follow a replayed graph)."""
    _lib.check(_lib.load().drba_conv_state_reset(_stream()), "drba_conv_state_reset")


def _pack_once(nfloats, pack, what, device):
    """The "pack on first use" step of every weight holder: `nfloats` host floats filled by `pack(dst)` (a *_pack entry point), then
    moved to `device`.  The holder keeps the result."""
    buf = torch.empty(nfloats, dtype=torch.float32)
    _lib.check(pack(C.c_void_p(buf.data_ptr())), what)
    return buf.to(device)


def _prune(packed, keep):
    """Drop the packings of the losing candidates: a tuner's warm launches pack the weights for every configuration it times."""
    for c in [c for c in packed if c not in keep]:
        del packed[c]


class _ConvLayer:
    """What Conv3x3 and Deconv4x4 share: the weights packed per kernel configuration on first use and the choice of that
    configuration (forced, tuned, or the library's cost model).  KIND names the entry points (drba_<KIND>_pack, ...).  A layer
    adds, for an [n, cin, h, w] input: _tune_key, _tune_stride, _pick_cfg, _out_hw / _out_shape and
    _work(cfg, n, h, w) -> (FLOP, the trace label's key) of its one launch."""

    def __init__(self, weight, bias, device, cfg, pre_slope):
        self.force_cfg = cfg  # tests only: pin a kernel configuration
        self.pre_slope = None if pre_slope is None else float(pre_slope)
        self.w_host = weight.detach().float().cpu().contiguous()
        self.two_term_ok = two_term_ok(self.w_host)  # False: family 4 is not offered to this layer
        self.device = device
        self.bias = None if bias is None else bias.detach().float().to(device).contiguous()
        self._packed, self._keep = {}, set()

    def _pack(self, cfg):
        if cfg not in self._packed:
            lib = _lib.load()
            n = getattr(lib, f"drba_{self.KIND}_packed_floats")(self.cin, self.cout, cfg)
            self._packed[cfg] = _pack_once(n, lambda dst: getattr(lib, f"drba_{self.KIND}_pack")(
                C.c_void_p(self.w_host.data_ptr()), dst, self.cin, self.cout, cfg), f"drba_{self.KIND}_pack", self.device)
        return self._packed[cfg]

    def _known_cfg(self, n, h, w):
        """The configuration a call on an [n, cin, h, w] input runs with, without tuning anything: the forced one, the tuner's
        winner (None: not tuned yet) or the cost model's pick."""
        if self.force_cfg is not None:
            return self.force_cfg
        if AUTOTUNE:
            return _tuned_get(self._tune_key(n, h, w), _families(self.two_term_ok))
        return self._pick_cfg(h, w)

    def _choose_cfg(self, x, run):
        """The configuration for this call on `x`; with the tuner on, the first call for a shape times `run(cfg)` for every candidate."""
        n, _, h, w = x.shape
        if self.force_cfg is not None:
            cfg = self.force_cfg
        elif AUTOTUNE and x.is_cuda:
            fam = _families(self.two_term_ok)
            cands = _candidates(_lib.load(), self.KIND, self._tune_stride(), fam, self.cin, self.cout)
            cfg = _tune(self._tune_key(n, h, w), cands, run, families=fam, persist=True, device=x.device.index,
                        pick=lambda: self._pick_cfg(h, w))
            self._keep.add(cfg)  # a layer can have one winner per batch size (block0: N=1 in calc_flow, N=2 stacked)
            _prune(self._packed, self._keep)
        else:
            cfg = self._pick_cfg(h, w)
        _lib.check(min(cfg, 0), f"drba_{self.KIND}_pick_cfg")
        return cfg


class Conv3x3(_ConvLayer):
    """One 3x3 conv layer (pad 1) with fused epilogue; weights are packed per kernel config on first use."""

    KIND = "conv3x3"
    ACTS = {None: 0, False: 0, "none": 0, True: 1, "lrelu": 1, "prelu": 2, "relu": 3, "tanh10": 4}

    def __init__(self, weight, bias, stride=1, act=True, beta=None, device=None, cfg=None, pre_slope=None,
                 post_slope=0.0):
        """act: True/'lrelu' LeakyReLU(0.2), 'prelu' (post_slope), 'relu', 'tanh10', None.  pre_slope: a float applies
        PReLU with that shared slope to the input inside the loader."""
        super().__init__(weight, bias, device, cfg, pre_slope)
        self.cout, self.cin = self.w_host.shape[:2]
        self.post_slope = float(post_slope)
        self.beta = None if beta is None else beta.detach().float().reshape(-1).to(device).contiguous()
        self.stride, self.act = int(stride), self.ACTS[act]

    def _out_hw(self, h, w):
        return (h - 1) // self.stride + 1, (w - 1) // self.stride + 1

    def _out_shape(self, n, h, w):
        return (n, self.cout, *self._out_hw(h, w))

    def _tune_key(self, n, h, w):
        return ("conv3x3", n, self.cin, self.cout, h, w, self.stride)

    def _tune_stride(self):
        return self.stride

    def _pick_cfg(self, h, w):
        return _lib.load().drba_conv3x3_pick_cfg(self.cin, self.cout, *self._out_hw(h, w), self.stride)

    def _work(self, cfg, n, h, w):
        ho, wo = self._out_hw(h, w)
        return 2.0 * self.cout * self.cin * 9 * ho * wo * n, (cfg, self.cin, self.cout, ho, wo, self.stride, n)

    def __call__(self, x, residual=None, out=None, residual2=None):
        x = _f32(x)
        n, cin, h, w = x.shape
        assert cin == self.cin, (cin, self.cin)
        lib = _lib.load()
        if out is None:
            out = torch.empty(self._out_shape(n, h, w), dtype=torch.float32, device=x.device)
        if self.beta is not None:
            assert residual is not None
        res = None if residual is None else _f32(residual)
        res2 = None if residual2 is None else _f32(residual2)
        pre, ps = (0, 0.0) if self.pre_slope is None else (1, self.pre_slope)
        run = lambda c: lib.drba_conv3x3(_p(x), _p(self._pack(c)), _p(self.bias), _p(self.beta), _p(res), _p(res2), _p(out), n, cin, h, w,  # noqa: E731
                                         self.cout, self.stride, self.act, self.post_slope, pre, ps, c, _stream())
        cfg = self._choose_cfg(x, run)
        work, key = self._work(cfg, n, h, w)
        _lib.check(_timed("conv3x3", key, work, "flop", lambda: run(cfg)), "drba_conv3x3")
        return out


def conv3x3_shuffle(layer, x):
    """pixel_shuffle2(layer(x)) with the shuffle in the convolution's store (drba_conv3x3_shuffle: GridNet's tail, 2 x 1.1 GB of
    traffic per 1080p frame less).  The configurations that carry the store form are a subset of family 4: when none of them
    accepts the layer (family 4 off, weights out of its range, ragged width) the two kernels run as before."""
    x = _f32(x)
    n, cin, h, w = x.shape
    lib = _lib.load()
    usable = (layer.stride == 1 and layer.pre_slope is None and layer.beta is None and layer.cout % 4 == 0 and w % 4 == 0
              and x.is_cuda and AUTOTUNE and layer.force_cfg is None and 4 in _families(layer.two_term_ok))
    if not usable:
        return pixel_shuffle2(layer(x))
    out = torch.empty((n, layer.cout // 4, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    cands = _candidates(lib, "conv3x3", 1, (4,), layer.cin, layer.cout)
    run = lambda c: lib.drba_conv3x3_shuffle(_p(x), _p(layer._pack(c)), _p(layer.bias), _p(out), n, cin, h, w, layer.cout,  # noqa: E731
                                             layer.act, layer.post_slope, c, _stream())
    try:
        cfg = _tune(("conv3x3_shuffle", n, cin, layer.cout, h, w), cands, run, families=(4,), persist=True, device=x.device.index,
                    pick=lambda: layer._pick_cfg(h, w))
    except NoKernelConfig:  # remembered per shape (in the process and in the store): the next call comes here without a launch
        _prune(layer._packed, layer._keep)
        return pixel_shuffle2(layer(x))
    layer._keep.add(cfg)
    _prune(layer._packed, layer._keep)
    _lib.check(_timed("conv3x3", (cfg, cin, layer.cout, h, w, 1, n, "ps"), 2.0 * layer.cout * cin * 9 * h * w * n, "flop", lambda: run(cfg)),
               "drba_conv3x3_shuffle")
    return out


class Deconv4x4(_ConvLayer):
    """ConvTranspose2d(k=4, s=2, p=1), optionally fused with PixelShuffle(2)."""

    KIND = "deconv4x4"

    def __init__(self, weight, bias, pixel_shuffle=False, device=None, cfg=None, pre_slope=None):
        super().__init__(weight, bias, device, cfg, pre_slope)
        self.cin, self.cout = self.w_host.shape[:2]  # [Cin, Cout, 4, 4]
        self.ps = 1 if pixel_shuffle else 0

    def _out_hw(self, h, w):
        """What a next layer of a chain would read: the transposed convolution's own output.  With PixelShuffle the layer's output is
        _out_shape's [n, cout/4, 4h, 4w], which this does NOT describe: such a layer is valid as the LAST layer of a chain only."""
        return 2 * h, 2 * w

    def _out_shape(self, n, h, w):
        return (n, self.cout // 4, 4 * h, 4 * w) if self.ps else (n, self.cout, 2 * h, 2 * w)

    def _tune_key(self, n, h, w):
        return ("deconv4x4", n, self.cin, self.cout, h, w, self.ps)

    def _tune_stride(self):
        return None  # (the transposed convolution's configuration ids carry no stride)

    def _pick_cfg(self, h, w):
        return _lib.load().drba_deconv4x4_pick_cfg(self.cin, self.cout, h, w)

    def _work(self, cfg, n, h, w):
        return 2.0 * self.cout * self.cin * 16 * h * w * n, (cfg, self.cin, self.cout, h, w, 2, n)

    def __call__(self, x, out=None):
        x = _f32(x)
        n, cin, h, w = x.shape
        assert cin == self.cin
        lib = _lib.load()
        if out is None:
            out = torch.empty(self._out_shape(n, h, w), dtype=torch.float32, device=x.device)
        pre, ps_ = (0, 0.0) if self.pre_slope is None else (1, self.pre_slope)
        run = lambda c: lib.drba_deconv4x4s2(_p(x), _p(self._pack(c)), _p(self.bias), _p(out), n, cin, h, w,  # noqa: E731
                                             self.cout, self.ps, pre, ps_, c, _stream())
        cfg = self._choose_cfg(x, run)
        work, key = self._work(cfg, n, h, w)
        _lib.check(_timed("deconv4x4", key, work, "flop", lambda: run(cfg)), "drba_deconv4x4s2")
        return out


class ConvChain:
    """A fixed sequence of Conv3x3 / Deconv4x4 layers (`residual=True` entries are ResConv layers adding their own
    input) issued by ONE library call (drba_conv_chain): the host cost of an IFBlock core drops from eleven
    Python/ctypes round trips to one.  A call for a shape some layer has no configuration for yet runs layer by layer (that
    is where the autotuner picks each layer's configuration), and so does every call of a chain that has a layer the
    library call cannot express (a pre_slope / post_slope) and every call on CPU tensors.  A traced call (bench.py's
    per-launch timing) is the same library call: the library records one launch per layer and the plan carries their tags."""

    def __init__(self, layers):
        self.layers = [(l, bool(r)) for l, r in layers]  # (layer, residual)
        self._plans = {}

    def _eager(self, x, out=None):
        for i, (layer, res) in enumerate(self.layers):
            o = out if i == len(self.layers) - 1 else None
            x = layer(x, residual=x, out=o) if res else layer(x, out=o)
        return x

    def _plan(self, n, h, w, device):
        descs = (_lib.ConvLayer * len(self.layers))()
        keep, sizes, tags = [], [], []
        for d, (layer, res) in zip(descs, self.layers):
            deconv = isinstance(layer, Deconv4x4)
            cfg = layer._known_cfg(n, h, w)
            if cfg is None or layer.pre_slope is not None or (not deconv and layer.post_slope != 0.0):
                return None
            if deconv:
                d.deconv, d.pixel_shuffle, d.stride, d.act, d.residual = 1, layer.ps, 1, 0, 0
            else:
                d.deconv, d.pixel_shuffle, d.stride, d.act, d.residual = 0, 0, layer.stride, layer.act, 1 if res else 0
                d.beta = 0 if layer.beta is None else layer.beta.data_ptr()
            work, key = layer._work(cfg, n, h, w)
            tags.append((work, "flop", f"{layer.KIND} {key}"))
            out_shape = layer._out_shape(n, h, w)
            sizes.append(math.prod(out_shape))  # (the scratch buffers hold the widest tensor between two layers)
            h, w = layer._out_hw(h, w)
            layer._keep.add(cfg)
            wp = layer._pack(cfg)
            keep.append(wp)
            d.packed_w, d.bias = wp.data_ptr(), (0 if layer.bias is None else layer.bias.data_ptr())
            d.cin, d.cout, d.cfg = layer.cin, layer.cout, cfg
        return {"descs": descs, "keep": keep, "scratch": max(sizes[:-1]) if len(sizes) > 1 else 0, "out_shape": out_shape,
                "bufs": {}, "tags": tags}

    def __call__(self, x, out=None):
        """out (optional): a contiguous float32 destination of the chain's output shape (a batch slice of a larger tensor)."""
        x = _f32(x)
        n, _, h, w = x.shape
        key = (n, h, w, "det") if deterministic() else (n, h, w)  # a plan holds configurations: one per mode
        plan = self._plans.get(key)
        if plan is None and key in self._plans:  # known: not chainable
            return self._eager(x, out)
        if not x.is_cuda:
            return self._eager(x, out)
        if plan is None:
            plan = self._plans[key] = self._plan(n, h, w, x.device)
            if plan is None:
                if AUTOTUNE:
                    del self._plans[key]  # configurations not tuned yet: this eager call tunes them, retry next time
                return self._eager(x, out)
        stream = _stream()
        bufs = plan["bufs"].get(stream.value)
        if bufs is None:  # scratch per stream: the same block runs on the main and on the lookahead stream
            m = max(plan["scratch"], 1)
            bufs = plan["bufs"][stream.value] = (torch.empty(m, dtype=torch.float32, device=x.device),
                                                 torch.empty(m, dtype=torch.float32, device=x.device))
        if out is None:
            out = torch.empty(plan["out_shape"], dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != tuple(plan["out_shape"]) or not out.is_contiguous() or out.dtype != torch.float32:
            raise _lib.DrbaHipError("ConvChain: out must be a contiguous float32 tensor of the chain's output shape")
        first = _trace_pos()
        _lib.check(_lib.load().drba_conv_chain(_p(x), _p(out), _p(bufs[0]), _p(bufs[1]), plan["descs"], len(self.layers), n,
                                               h, w, stream), "drba_conv_chain")
        _tag(first, plan["tags"])  # one launch per layer, in order
        return out


# ----------------------------------------------------------------------------- IFNet glue
PAIR_FEATURES = True  # warped stages read the encoder features from a pair-interleaved copy (half the gather instructions)


HEAD_TWO_TERM = None  # None: follow CONV_FAMILIES (family 4 allowed -> head_fused16.hip); True / False force it (tests, A/B)
HEAD_FUSED = True  # IFNet's encoder as one kernel (drba_head_fused) instead of four layers + the pair-interleave copy (tools/ab_bench.py --no-head-fused: A/B)


def head_fused(img, layers, holder, planar=True):
    """Head(img) (IFNet_HDv3.py:23-47) in one launch: layers = (cnn0, cnn1, cnn2 Conv3x3, cnn3 Deconv4x4); returns f [1,16,H,W]
    with its pair-interleaved copy already attached (pair_interleaved(f) costs nothing afterwards).  planar=False (the hot
    path: RIFE's own calls): ONLY the pair-interleaved layout [8,H,W,2] is written and returned, tagged as such -- every
    kernel of the pipeline reads that layout, and the planar copy is 134 MB of HBM writes per 1080p frame nobody reads;
    features_planar() converts where a caller wants the reference's [1,16,H,W].  `holder` keeps the packed weights.  None
    when the shape is not one the kernel takes (odd sizes, a batch)."""
    img = _f32(img)
    n, c, H, W = img.shape
    if n != 1 or c != 3 or H % 2 or W % 4:
        return None
    lib = _lib.load()
    # the two-term fp16 form of the kernel (head_fused16.hip) when the conv tuner may use kernel family 4, else fp32 MFMA
    two = _two_term(HEAD_TWO_TERM, all(l.two_term_ok for l in layers))
    attr, sfx = ("_fused_pack16", "16") if two else ("_fused_pack", "")
    launch = getattr(lib, "drba_head_fused" + sfx)
    pk = getattr(holder, attr, None)
    if pk is None:
        src = [t for l in layers for t in (l.w_host, l.bias.detach().float().cpu().contiguous())]  # weight, bias of each layer in turn
        pk = _pack_once(getattr(lib, f"drba_head_fused{sfx}_packed_floats")(), lambda dst: getattr(lib, f"drba_head_fused{sfx}_pack")(
            *(C.c_void_p(t.data_ptr()) for t in src), dst), f"drba_head_fused{sfx}_pack", img.device)
        setattr(holder, attr, pk)
    f = torch.empty((1, 16, H, W), dtype=torch.float32, device=img.device) if planar else None
    fp = torch.empty((8, H, W, 2), dtype=torch.float32, device=img.device)
    # algorithmic bytes: the frame read, the features written in both layouts; 9.5 GFLOP of fp32 MFMA work per 1080p frame
    # ride along (61 us at the fp32 MFMA peak against 50 us of HBM time: the matrix cores are the binding roofline)
    flop = 2.0 * (16 * 27 + 2 * 16 * 144) * (H // 2) * (W // 2) + 2.0 * 16 * 16 * 16 * (H // 2) * (W // 2)
    _lib.check(_timed("head_fused" + sfx, (H, W), flop, "flop", lambda: launch(_p(img), _p(pk), _p(f), _p(fp), 1, H, W, _stream())),
               "drba_head_fused" + sfx)
    if not planar:
        fp._drba_is_pair = True
        return fp
    _set_copy(f, "_drba_pair", fp, versioned=False)
    return f


def is_pair(f):
    """Is `f` a feature tensor in the pair-interleaved layout [C/2,H,W,2] (head_fused(planar=False))?  The tag does not survive
    a .clone() / slice of a carried `reuse` entry, so the SHAPE decides as well: [8,H,W,2] cannot be the reference's
    [1,16,H,W] (a planar tensor handed to the kernels as pairs, or the reverse, would be read in the wrong layout silently)."""
    if getattr(f, "_drba_is_pair", False):
        return True
    return bool(torch.is_tensor(f) and f.dim() == 4 and f.shape[0] == 8 and f.shape[3] == 2 and f.shape[1] > 2 and f.shape[2] > 2)


def features_planar(f):
    """The reference's layout [1,16,H,W] of a feature tensor (tests, callers that inspect `reuse`); pair-only tensors are
    converted (a torch view + copy: not on the hot path)."""
    if not is_pair(f):
        return f
    c2, h, w, _ = f.shape
    return f.permute(0, 3, 1, 2).reshape(1, 2 * c2, h, w).contiguous()


def _feat(f, want_pair=True):
    """-> (planar tensor or None, pair-interleaved tensor or None) of a feature argument."""
    if is_pair(f):
        if not (f.is_cuda and f.dtype == torch.float32 and f.is_contiguous()):
            raise _lib.DrbaHipError("pair-interleaved features must be a contiguous float32 CUDA tensor [8,H,W,2]")
        return None, f
    f = _f32(f)
    if f.dim() != 4 or f.shape[0] != 1:
        raise _lib.DrbaHipError(f"features must be [1,C,H,W] (or pair-interleaved [8,H,W,2]), got {tuple(f.shape)}")
    return f, (pair_interleaved(f) if want_pair and PAIR_FEATURES and f.shape[1] == 16 else None)


def _feat2(f0, f1, want_pair=True):
    """_feat of both feature arguments of an item, in ONE layout: when one of them exists pair-interleaved only (the hot path's
    tensors) and the other is planar (a reference / oracle `reuse` entry), the planar one is given its pair copy and the
    kernels read pairs -- the C entry points take the planar pointers of an item both or not at all."""
    (a, ap), (b, bp) = _feat(f0, want_pair), _feat(f1, want_pair)
    if a is None or b is None:
        ap = ap if ap is not None else pair_interleaved(a)
        bp = bp if bp is not None else pair_interleaved(b)
        a = b = None
    return (a, ap), (b, bp)


def _feat_batch(items, want_pair=True):
    """_feat2 for every (.., f0, f1) item of a batched launch, all items in ONE layout (the C entry points want the items of a
    launch to agree on which pointers are given): if any item is pair-only, every item is read as pairs."""
    fs = [_feat2(it[3], it[4], want_pair) for it in items]
    if any(a is None for (a, _), _ in fs):
        fs = [((None, ap if ap is not None else pair_interleaved(a)), (None, bp if bp is not None else pair_interleaved(b)))
              for (a, ap), (b, bp) in fs]
    return fs


def pair_interleaved(f):
    """[1,C,H,W] -> the [C/2,H,W,2] copy the stage-input gathers read; made once per feature tensor and kept on it."""
    if is_pair(f):
        return f
    fp = _copy_of(f, "_drba_pair", versioned=False)
    if fp is None:
        n, c, h, w = f.shape
        fp = torch.empty((c // 2, h, w, 2), dtype=torch.float32, device=f.device)
        _lib.check(_timed("pair_interleave", (c, h, w), 8.0 * c * h * w, "byte", lambda: _lib.load().drba_pair_interleave(
            _p(f), _p(fp), c, h, w, _stream())), "drba_pair_interleave")
        _set_copy(f, "_drba_pair", fp, versioned=False)
    return fp


IMG_X4 = True  # the gathers read the frames from their [H,W,4] copies (two 16-byte loads per tap row instead of three 8-byte ones)


def _x4_of(img):
    """The [H,W,4] copy a frame carries (ops.to_inp writes it with the frame; rgbx() makes it on demand), or None: then the
    kernels read the planes.  A frame that did not come from to_inp (tests, a caller's own tensors) is NOT converted behind the
    caller's back per call -- rgbx(frame) once is the caller's choice."""
    return _copy_of(img, "_drba_x4") if IMG_X4 else None


def rgbx(img):
    """A frame [1,3,H,W] -> its [H,W,4] copy (c0, c1, c2, 0), made once per tensor (to_inp writes it with the frame) and kept on it."""
    x4 = _copy_of(img, "_drba_x4")
    if x4 is None:
        _, _, h, w = img.shape
        x4 = torch.empty((h, w, 4), dtype=torch.float32, device=img.device)
        _lib.check(_timed("rgbx", (h, w), 28.0 * h * w, "byte", lambda: _lib.load().drba_rgbx(_p(img), _p(x4), h, w, _stream())), "drba_rgbx")
        _set_copy(img, "_drba_x4", x4)
    return x4


def _stage_geometry(H, W, scale):
    """-> (h, w, pts): a stage's resolution at 1/scale and the full-resolution sample points its gather reads per channel
    (every pixel at scale <= 2, a 2x2 footprint per output point above)."""
    h, w = int(np.floor(H * (1.0 / scale))), int(np.floor(W * (1.0 / scale)))
    return h, w, (H * W if scale <= 2 else 4 * h * w)


def _timestep(t):
    """A timestep argument -> (its [1,1,H,W] map or None, its scalar value)."""
    return (_f32(t), 0.0) if torch.is_tensor(t) else (None, float(t))


# algorithmic bytes of a stage input per item: every full-resolution sample point read once per full-resolution channel (the 9
# channels of mask / feat and flow come from the low-resolution head output) + the output written (+ the folded flow)
def _input_bytes(nch, has_flow, pts, h, w):
    return 4.0 * ((nch - (9 if has_flow else 0)) * pts + nch * h * w)


def _input_lds_bytes(pts, h, w, fold):
    return 4.0 * (43 * pts + 52 * h * w + (4 * pts if fold else 0))


def ifblock_input(img0, img1, f0, f1, timestep, flow, tmp_prev, prev_scale, scale, out=None):
    """Stage input at 1/scale resolution (52 ch with flow, 39 without).  `timestep`: float or [1,1,H,W] map;
    `tmp_prev`: the previous stage's [1,13,hp,wp] head output (mask/feat are its x prev_scale upsample).
    `out`: optional [1,nch,h,w] destination (one sample of a stacked stage batch)."""
    img0, img1 = _f32(img0), _f32(img1)
    (f0, f0p), (f1, f1p) = _feat2(f0, f1, flow is not None)
    _, _, H, W = img0.shape
    h, w, pts = _stage_geometry(H, W, scale)
    tmap, tsc = _timestep(timestep)
    nch = 52 if flow is not None else 39
    if out is None:
        out = torch.empty((1, nch, h, w), dtype=torch.float32, device=img0.device)
    elif tuple(out.shape) != (1, nch, h, w) or not out.is_contiguous():
        raise _lib.DrbaHipError(f"ifblock_input: out must be a contiguous [1,{nch},{h},{w}] tensor")
    hp = wp = 0
    ps = 1.0
    if flow is not None:
        flow, tmp_prev = _f32(flow), _f32(tmp_prev)
        hp, wp, ps = tmp_prev.shape[2], tmp_prev.shape[3], float(prev_scale)
    lib = _lib.load()
    nbytes = _input_bytes(nch, flow is not None, pts, h, w)
    _lib.check(_timed("ifblock_input", (nch, H, W, h, w), nbytes, "byte", lambda: lib.drba_ifblock_input(
        _p(img0), _p(img1), _p(f0), _p(f1), _p(f0p), _p(f1p), _p(tmap), tsc, _p(flow), _p(tmp_prev), hp, wp, ps, _p(out), H, W, h, w,
        float(scale), _stream())), "drba_ifblock_input")
    return out


LDS_STAGE_INPUT = True  # warped stage inputs through drba_ifblock_input_lds (tmp_prev's footprint staged in LDS)


def ifblock_input_lds(img0, img1, f0, f1, timestep, flow, tmp_prev, prev_scale, scale, out=None, fold=False):
    """Warped stage input like ifblock_input(flow != None), previous head output staged through LDS.  fold=True: `flow` is
    the running flow BEFORE the previous stage's update (or None); the update flow + up(tmp_prev[:4]) * prev_scale is
    formed inside the kernel (scale <= 2 only) and returned as the second value."""
    img0, img1, tmp_prev = _f32(img0), _f32(img1), _f32(tmp_prev)
    (f0, f0p), (f1, f1p) = _feat2(f0, f1)
    _, _, H, W = img0.shape
    h, w, pts = _stage_geometry(H, W, scale)
    tmap, tsc = _timestep(timestep)
    if out is None:
        out = torch.empty((1, 52, h, w), dtype=torch.float32, device=img0.device)
    elif tuple(out.shape) != (1, 52, h, w) or not out.is_contiguous():
        raise _lib.DrbaHipError(f"ifblock_input_lds: out must be a contiguous [1,52,{h},{w}] tensor")
    flow = None if flow is None else _f32(flow)
    flow_out = torch.empty((1, 4, H, W), dtype=torch.float32, device=img0.device) if fold else None
    hp, wp = tmp_prev.shape[2], tmp_prev.shape[3]
    lib = _lib.load()
    nbytes = _input_lds_bytes(pts, h, w, fold)
    _lib.check(_timed("ifblock_input_lds" + ("+fold" if fold else ""), (52, H, W, h, w), nbytes, "byte", lambda: lib.drba_ifblock_input_lds(
        _p(img0), _p(img1), _p(f0), _p(f1), _p(f0p), _p(f1p), _p(tmap), tsc, _p(flow), _p(tmp_prev), hp, wp, float(prev_scale),
        _p(flow_out), _p(out), H, W, h, w, float(scale), _stream())), "drba_ifblock_input_lds")
    return (out, flow_out) if fold else out


def _ptr(t):
    return None if t is None else t.data_ptr()


LAZY_FLOW = True  # IFNet's running flow as a list of terms (earlier head outputs) evaluated inside the consumers instead of a
#                   full-resolution tensor updated after every stage (drba_hip.h drba_flow_terms_t; tools/ab_bench.py --no-lazy-flow: A/B)


def _flow_terms(terms, B):
    """terms: [(head output [B,13,h,w], stage scale), ...] oldest first -> (ctypes drba_flow_terms_t, the float32 tensors)."""
    if len(terms) > _lib.MAX_FLOW_TERMS:
        raise _lib.DrbaHipError(f"at most {_lib.MAX_FLOW_TERMS} flow terms")
    ft = _lib.FlowTerms()
    ft.n = len(terms)
    ts = []
    for i, (t, s) in enumerate(terms):
        t = _f32(t)
        if t.shape[0] != B or t.shape[1] != 13:
            raise _lib.DrbaHipError(f"flow term {i}: expected [{B},13,h,w], got {tuple(t.shape)}")
        ft.h[i], ft.w[i], ft.scale[i] = t.shape[2], t.shape[3], float(s)
        ts.append(t)
    return ft, ts


def _frames(items, what):
    """The two float32 frames of every item of a batched launch -> [(img0, img1), ...]."""
    if len(items) > _lib.MAX_STAGE_ITEMS:
        raise _lib.DrbaHipError(f"{what}: at most {_lib.MAX_STAGE_ITEMS} items per launch")
    return [(_f32(it[0]), _f32(it[1])) for it in items]


def _x4_pair(i0, i1):
    """The [H,W,4] copies of an item's two frames where BOTH carry one (the kernels take an item's two pointers or neither), else None."""
    x0, x1 = _x4_of(i0), _x4_of(i1)
    return None if x0 is None or x1 is None else (x0, x1)


def _stage_items(imgs, x4, out, tmp_prev, terms=(), feats=None, timesteps=None, flows=None, flow_out=None):
    """The drba_stage_item_t[B] of a batched launch -> (the ctypes array, the tensors its pointers need alive beyond the caller's own).
    imgs: _frames(items); x4: per item its _x4_pair or None (WHICH items get their copies is the caller's rule); out, tmp_prev,
    flow_out and every tensor of `terms` are stacked [B, ...] tensors and item k takes their slice k; feats: _feat_batch(items);
    timesteps: per item a float or a map; flows: per item the running flow or None."""
    arr, keep = (_lib.StageItem * len(imgs))(), []
    for k, (i0, i1) in enumerate(imgs):
        a = arr[k]
        a.img0, a.img1, a.out = i0.data_ptr(), i1.data_ptr(), out[k].data_ptr()
        a.tmp_prev = None if tmp_prev is None else tmp_prev[k].data_ptr()
        a.flow_out = None if flow_out is None else flow_out[k].data_ptr()
        keep += [i0, i1]
        if feats is not None:
            (f0, f0p), (f1, f1p) = feats[k]
            tmap, tsc = _timestep(timesteps[k])
            fl = None if (flows is None or flows[k] is None) else _f32(flows[k])
            a.f0, a.f1, a.f0_pair, a.f1_pair = _ptr(f0), _ptr(f1), _ptr(f0p), _ptr(f1p)
            a.timestep_map, a.timestep_scalar, a.flow = _ptr(tmap), tsc, _ptr(fl)
            keep += [f0, f1, f0p, f1p, tmap, fl]
        if x4[k] is not None:
            a.img0_x4, a.img1_x4 = x4[k][0].data_ptr(), x4[k][1].data_ptr()
            keep += x4[k]
        for i, t in enumerate(terms):
            a.term[i] = t[k].data_ptr()
    return arr, keep


def stage_inputs(items, flows, tmp_prev, prev_scale, scale, out, fold=False, lds=True, terms=None):
    """The stage input of EVERY item of a stage in one launch (drba_ifblock_input[_lds]_batch).
    items: [(img0, img1, timestep, f0, f1), ...]; flows: per-item running flow (or None); tmp_prev: the previous stage's
    stacked head output [B,13,hp,wp] (or None at the first stage); out: the stacked [B,nch,h,w] stage input.
    fold=True (lds only): returns the list of folded running flows (slices of one new [B,4,H,W] tensor).
    terms (lds only, instead of flows / fold): the running flow BEFORE tmp_prev's update as [(head output [B,13,h,w], scale), ...]
    of the earlier stages, oldest first; the kernel forms flow = sum(terms) + up(tmp_prev[:, :4]) * prev_scale at its sample
    points (drba_ifblock_input_lazy_batch) and nothing but `out` is written."""
    B = len(items)
    imgs = _frames(items, "stage_inputs")
    lazy = terms is not None
    if lazy and (flows is not None or fold or not lds):
        raise _lib.DrbaHipError("stage_inputs: terms replace flows / fold (lds path only)")
    ft, tts = _flow_terms(terms, B) if lazy else (None, [])
    _, _, H, W = imgs[0][0].shape
    h, w, pts = _stage_geometry(H, W, scale)
    has_flow = flows is not None and flows[0] is not None
    nch = 52 if (has_flow or lds) else 39
    if tuple(out.shape) != (B, nch, h, w) or not out.is_contiguous():
        raise _lib.DrbaHipError(f"stage_inputs: out must be a contiguous [{B},{nch},{h},{w}] tensor")
    if lazy and tmp_prev is None:
        raise _lib.DrbaHipError("stage_inputs: terms need tmp_prev (the newest head output)")
    flow_out = torch.empty((B, 4, H, W), dtype=torch.float32, device=imgs[0][0].device) if fold else None
    hp = wp = 0
    ps = 1.0
    if tmp_prev is not None:
        tmp_prev = _f32(tmp_prev)
        hp, wp, ps = tmp_prev.shape[2], tmp_prev.shape[3], float(prev_scale)
    # the [H,W,4] copies per item, where both of its frames carry one -- on the LDS path at scale <= 2 only: the sparser sample points of the
    # coarser stages put a quad of lanes on more cache lines with 16-byte pixels (same box: scale 4 313-318 us against 309-312, scale 8 153 against 148)
    x4 = [_x4_pair(i0, i1) if lds and scale <= 2 else None for i0, i1 in imgs]
    arr, keep = _stage_items(imgs, x4, out, tmp_prev, tts, _feat_batch(items, lds or has_flow), [it[2] for it in items], flows, flow_out)
    lib = _lib.load()
    if lazy:
        nbytes = B * 4.0 * (39 * pts + 52 * h * w)  # no flow read, none written: the terms are a few KB per tile
        _lib.check(_timed("ifblock_input_lds+lazy", (52, H, W, h, w, B), nbytes, "byte",
                          lambda: lib.drba_ifblock_input_lazy_batch(C.cast(arr, C.c_void_p), B, C.cast(C.pointer(ft), C.c_void_p), hp, wp, ps, H, W, h, w,
                                                                    float(scale), _stream())), "drba_ifblock_input_lazy_batch")
        return None
    if lds:
        _lib.check(_timed("ifblock_input_lds" + ("+fold" if fold else ""), (52, H, W, h, w, B), B * _input_lds_bytes(pts, h, w, fold), "byte",
                          lambda: lib.drba_ifblock_input_lds_batch(C.cast(arr, C.c_void_p), B, hp, wp, ps, H, W, h, w, float(scale),
                                                                   _stream())), "drba_ifblock_input_lds_batch")
    else:
        _lib.check(_timed("ifblock_input", (nch, H, W, h, w, B), B * _input_bytes(nch, has_flow, pts, h, w), "byte",
                          lambda: lib.drba_ifblock_input_batch(C.cast(arr, C.c_void_p), B, hp, wp, ps, H, W, h, w, float(scale),
                                                               _stream())), "drba_ifblock_input_batch")
    return [flow_out[k:k + 1] for k in range(B)] if fold else None


STAGE_CONV_FUSED = True  # the scale-1 stage input and the IFBlock's first convolution in one kernel (tools/ab_bench.py --no-stage-conv: A/B)
STAGE_CONV_TWO_TERM = None  # None: follow CONV_FAMILIES (family 4 allowed -> stage_conv16.hip); True / False force it (tests, A/B)


def _stage_conv_two_term(conv):
    return _two_term(STAGE_CONV_TWO_TERM, conv.two_term_ok)


STAGE_CONV_S2 = True  # the scale-2 stage fused the same way (stage_conv16_s2; A/B: tools/ab_bench.py --no-stage-conv-s2)


def stage_conv0_ok(conv, H, W, scale, prev_scale, items=None):
    """Can drba_stage_conv{0,16}_batch replace stage_inputs(scale) + conv (the IFBlock's first convolution)?  Scale 2 is taken by
    the two-term kernel only, for the lazy flow, when every frame of `items` carries its [H,W,4] copy (ops.to_inp / ops.rgbx)."""
    if not (STAGE_CONV_FUSED and PAIR_FEATURES and conv.cin == 52 and conv.stride == 2 and conv.act == 1 and conv.beta is None
            and conv.pre_slope is None and conv.post_slope == 0.0):
        return False
    lib = _lib.load()
    if float(scale) == 2.0:
        if not (STAGE_CONV_S2 and _stage_conv_two_term(conv) and items is not None
                and all(_x4_pair(_f32(it[0]), _f32(it[1])) is not None for it in items)):
            return False
    if _stage_conv_two_term(conv):
        return bool(lib.drba_stage_conv16_supported(H, W, float(scale), float(prev_scale), conv.cout))
    return bool(lib.drba_stage_conv0_supported(H, W, float(scale), float(prev_scale), conv.cout))  # 16 output channels only


def stage_conv0(items, flows, tmp_prev, prev_scale, conv, fold=False, terms=None, scale=1, out=None):
    """The scale-1 stage input of every item fused with `conv` (52 -> 16, stride 2, LeakyReLU): stage_inputs(..., scale=1)
    followed by conv(xin) without the 52-channel tensor (drba_stage_conv16_batch: two fp16 terms per operand, kernel family 4;
    drba_stage_conv0_batch: exact fp32 products, when family 4 is not allowed).  Returns (y0 [B,16,Ho,Wo], folded flows
    or None).  terms: as in stage_inputs (instead of flows / fold)."""
    B = len(items)
    lazy = terms is not None
    if lazy and (flows is not None or fold):
        raise _lib.DrbaHipError("stage_conv0: terms replace flows / fold")
    ft, tts = _flow_terms(terms, B) if lazy else (None, [])
    imgs = _frames(items, "stage_conv0")
    _, _, H, W = imgs[0][0].shape
    sc = int(scale)
    two = _stage_conv_two_term(conv)
    if sc not in (1, 2) or (sc == 2 and not (lazy and two)):
        raise _lib.DrbaHipError("stage_conv0: scale 1, or scale 2 with the flow as terms in the two-term form")
    hs, ws_ = H // sc, W // sc                              # the stage's resolution
    Ho, Wo = (hs - 1) // 2 + 1, (ws_ - 1) // 2 + 1          # the convolution's output
    dev = imgs[0][0].device
    attr = "_stage_pack16" if two else "_stage_pack"
    if getattr(conv, attr, None) is None:
        lib, w_host = _lib.load(), C.c_void_p(conv.w_host.data_ptr())
        if two:
            packed = _pack_once(lib.drba_stage_conv16_packed_floats(conv.cout), lambda dst: lib.drba_stage_conv16_pack(w_host, conv.cout, dst),
                                "drba_stage_conv16_pack", dev)
        else:
            packed = _pack_once(lib.drba_stage_conv0_packed_floats(), lambda dst: lib.drba_stage_conv0_pack(w_host, dst), "drba_stage_conv0_pack", dev)
        setattr(conv, attr, packed)
    packed = getattr(conv, attr)
    tmp_prev = _f32(tmp_prev)
    hp, wp = tmp_prev.shape[2], tmp_prev.shape[3]
    if out is None:
        out = torch.empty((B, conv.cout, Ho, Wo), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, conv.cout, Ho, Wo) or not out.is_contiguous() or out.dtype != torch.float32:  # a batch slice of a wider tensor
        raise _lib.DrbaHipError(f"stage_conv0: out must be a contiguous float32 [{B},{conv.cout},{Ho},{Wo}] tensor")
    flow_out = torch.empty((B, 4, H, W), dtype=torch.float32, device=dev) if fold else None
    x4 = [_x4_pair(i0, i1) for i0, i1 in imgs]
    if any(p is None for p in x4):  # the [H,W,4] copies for all items or for none (the items of a launch agree)
        x4 = [None] * B
    arr, keep = _stage_items(imgs, x4, out, tmp_prev, tts, _feat_batch(items), [it[2] for it in items], flows, flow_out)
    # algorithmic bytes: 43 source channels read once per full-resolution point, the 16-channel quarter-size output (and the
    # folded flow) written; 2 * 16 * 52 * 9 FLOP per output pixel ride along (50 us per 1080p sample at the fp32 MFMA peak,
    # 53 us of HBM time: the byte roofline is the binding one)
    nbytes = B * 4.0 * ((39.0 if lazy else 43.0) * H * W + conv.cout * Ho * Wo + (4.0 * H * W if fold else 0.0))
    bias = None if conv.bias is None else conv.bias.data_ptr()
    tptr = C.cast(C.pointer(ft), C.c_void_p) if lazy else None
    name = ("stage_conv16" if two else "stage_conv0") + ("_s2" if sc == 2 else "") + ("+fold" if fold else "+lazy" if lazy else "")
    if two:
        call = lambda: _lib.load().drba_stage_conv16_batch(C.cast(arr, C.c_void_p), B, tptr, hp, wp, float(prev_scale), H, W, float(sc),  # noqa: E731
                                                           conv.cout, packed.data_ptr(), bias, _stream())
    else:
        call = lambda: _lib.load().drba_stage_conv0_batch(C.cast(arr, C.c_void_p), B, tptr, hp, wp, float(prev_scale), H, W,  # noqa: E731
                                                          packed.data_ptr(), bias, _stream())
    _lib.check(_timed(name, (52, conv.cout, H, W, B), nbytes, "byte", call), "drba_stage_conv16_batch" if two else "drba_stage_conv0_batch")
    return out, ([flow_out[k:k + 1] for k in range(B)] if fold else None)


def flow_updates(tmp, flows, H, W, scale, whole=False):
    """flow_k + up(tmp[k][:4]) * scale for every item of a stage in one launch -> list of [1,4,H,W] (slices of one tensor;
    whole=True: that [B,4,H,W] tensor itself)."""
    tmp = _f32(tmp)
    B, c, h, w = tmp.shape
    out = torch.empty((B, 4, H, W), dtype=torch.float32, device=tmp.device)
    fin = [None if f is None else _f32(f) for f in flows]
    P3 = C.c_void_p * B
    a_tmp = P3(*[tmp[k].data_ptr() for k in range(B)])
    a_in = P3(*[_ptr(f) for f in fin])
    a_out = P3(*[out[k].data_ptr() for k in range(B)])
    _lib.check(_timed("ifblock_update", (h, w, H, W, B), B * 4.0 * (8.0 * H * W + 4.0 * h * w), "byte",
                      lambda: _lib.load().drba_ifblock_update_batch(C.cast(a_tmp, C.c_void_p), C.cast(a_in, C.c_void_p),
                                                                    C.cast(a_out, C.c_void_p), B, h, w, H, W, float(scale),
                                                                    _stream())), "drba_ifblock_update_batch")
    return out if whole else [out[k:k + 1] for k in range(B)]


def warp_blend_fold(img0, img1, flow_prev, tmp_last, scale):
    """Final frame with the last stage's flow update folded in (flow_prev: running flow before it, or None)."""
    img0, img1, tmp_last = _f32(img0), _f32(img1), _f32(tmp_last)
    flow_prev = None if flow_prev is None else _f32(flow_prev)
    _, _, H, W = img0.shape
    h, w = tmp_last.shape[2], tmp_last.shape[3]
    out = torch.empty((1, 3, H, W), dtype=torch.float32, device=img0.device)
    nbytes = 4.0 * ((6 + 4 + 3) * H * W + 5 * h * w)
    _lib.check(_timed("warp_blend_fold", (H, W), nbytes, "byte", lambda: _lib.load().drba_warp_blend_fold(
        _p(img0), _p(img1), _p(flow_prev), _p(tmp_last), h, w, float(scale), _p(out), H, W, _stream())), "drba_warp_blend_fold")
    return out


def warp_blend_lazy(items, terms, tmp_last, scale):
    """The final frames of every item of a stage in one launch, the flow before the last stage given as terms
    (drba_warp_blend_lazy_batch): items = [(img0, img1, ...), ...], tmp_last [B,13,h,w] -> list of [1,3,H,W]."""
    B = len(items)
    imgs = _frames(items, "warp_blend_lazy")
    tmp_last = _f32(tmp_last)
    ft, tts = _flow_terms(terms, B)
    _, _, H, W = imgs[0][0].shape
    h, w = tmp_last.shape[2], tmp_last.shape[3]
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=imgs[0][0].device)
    arr, keep = _stage_items(imgs, [_x4_pair(i0, i1) for i0, i1 in imgs], out, tmp_last, tts)  # the [H,W,4] copies per item
    nbytes = B * 4.0 * ((6 + 3) * H * W + 5 * h * w)
    _lib.check(_timed("warp_blend_lazy", (H, W, B), nbytes, "byte", lambda: _lib.load().drba_warp_blend_lazy_batch(
        C.cast(arr, C.c_void_p), B, C.cast(C.pointer(ft), C.c_void_p), h, w, float(scale), H, W, _stream())), "drba_warp_blend_lazy_batch")
    return [out[k:k + 1] for k in range(B)]


def ifblock_update(tmp, flow_in, H, W, scale, want_mask_feat=False):
    """flow (and optionally mask, feat) at full resolution from the 13-channel head output at 1/scale."""
    tmp = _f32(tmp)
    _, c, h, w = tmp.shape
    assert c == 13
    dev = tmp.device
    flow = torch.empty((1, 4, H, W), dtype=torch.float32, device=dev)
    mask = feat = None
    if want_mask_feat:
        mask = torch.empty((1, 1, H, W), dtype=torch.float32, device=dev)
        feat = torch.empty((1, 8, H, W), dtype=torch.float32, device=dev)
    if flow_in is not None:
        flow_in = _f32(flow_in)
    nbytes = 4.0 * (13 * h * w + (4 if flow_in is not None else 0) * H * W + (13 if want_mask_feat else 4) * H * W)
    _lib.check(_timed("ifblock_update", (h, w, H, W), nbytes, "byte", lambda: _lib.load().drba_ifblock_update(
        _p(tmp), _p(flow_in), _p(flow), _p(mask), _p(feat), h, w, H, W, float(scale), _stream())), "drba_ifblock_update")
    return (flow, mask, feat) if want_mask_feat else flow


def warp_blend(img0, img1, flow, tmp_last, scale):
    """Final frame from the two inputs, the accumulated flow and the last head output (mask = channel 4)."""
    img0, img1, flow, tmp_last = _f32(img0), _f32(img1), _f32(flow), _f32(tmp_last)
    _, _, H, W = img0.shape
    h, w = tmp_last.shape[2], tmp_last.shape[3]
    mask_lo = tmp_last[:, 4:5]  # contiguous plane of the [1,13,h,w] tensor
    out = torch.empty((1, 3, H, W), dtype=torch.float32, device=img0.device)
    nbytes = 4.0 * ((6 + 4 + 3) * H * W + h * w)
    _lib.check(_timed("warp_blend", (H, W), nbytes, "byte", lambda: _lib.load().drba_warp_blend(
        _p(img0), _p(img1), _p(flow), C.c_void_p(mask_lo.data_ptr()), h, w, float(scale), _p(out), H, W, _stream())),
        "drba_warp_blend")
    return out


# ----------------------------------------------------------------------------- GMFSS glue
def metric_input(img0, img1, flow01, flow10):
    img0, img1, flow01, flow10 = _f32(img0), _f32(img1), _f32(flow01), _f32(flow10)
    _, _, h, w = img0.shape
    out = torch.empty((1, 14, h, w), dtype=torch.float32, device=img0.device)
    _lib.check(_lib.load().drba_metric_input(_p(img0), _p(img1), _p(flow01), _p(flow10), _p(out), h, w, _stream()),
               "drba_metric_input")
    return out


def pixel_shuffle2(x):
    x = _f32(x)
    n, c4, h, w = x.shape
    assert c4 % 4 == 0
    out = torch.empty((n, c4 // 4, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    # (the samples of a batch are just more groups of 4 channels: [N, 4C, h, w] -> [N * C] output planes)
    _lib.check(_lib.load().drba_pixel_shuffle2(_p(x), _p(out), n * (c4 // 4), h, w, _stream()), "drba_pixel_shuffle2")
    return out


def timestep_fix(t0, t1, cover0, cover1):
    t0, t1, cover0, cover1 = _f32(t0), _f32(t1), _f32(cover0), _f32(cover1)
    o0, o1 = torch.empty_like(t0), torch.empty_like(t1)
    _lib.check(_lib.load().drba_timestep_fix(_p(t0), _p(t1), _p(cover0), _p(cover1), _p(o0), _p(o1), t0.numel(),
                                             _stream()), "drba_timestep_fix")
    return o0, o1


def swap_select(x, y, t0, t1, thr=25.0, out=None):
    """`out`: optional (ox, oy) destinations (contiguous, e.g. channel slices of a concatenation buffer)."""
    x, y, t0, t1 = _f32(x), _f32(y), _f32(t0), _f32(t1)
    n, c, h, w = x.shape
    assert n == 1 and t0.shape[2:] == x.shape[2:]
    ox, oy = (torch.empty_like(x), torch.empty_like(y)) if out is None else out
    if tuple(ox.shape) != tuple(x.shape) or tuple(oy.shape) != tuple(y.shape) or not (ox.is_contiguous() and oy.is_contiguous()):
        raise _lib.DrbaHipError("swap_select: out must be contiguous tensors of the inputs' shapes")
    _lib.check(_lib.load().drba_swap_select(_p(x), _p(y), _p(t0), _p(t1), _p(ox), _p(oy), c, h, w, float(thr),
                                            _stream()), "drba_swap_select")
    return ox, oy


def clamp(x, lo, hi):
    x = _f32(x)
    out = torch.empty_like(x)
    _lib.check(_lib.load().drba_clamp(_p(x), _p(out), float(lo), float(hi), x.numel(), _stream()), "drba_clamp")
    return out


# ----------------------------------------------------------------------------- GMFlow operators
def conv_direct(x, w, bias, stride, pad):
    x, w = _f32(x), _f32(w)
    n, cin, h, wd = x.shape
    cout, _, k, _ = w.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    out = torch.empty((n, cout, ho, wo), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().drba_conv_direct(_p(x), _p(w), _p(bias), _p(out), n, cin, h, wd, cout, k, stride, pad,
                                            _stream()), "drba_conv_direct")
    return out


def instance_norm(x, relu=False, eps=1e-5):
    x = _f32(x)
    n, c, h, w = x.shape
    out = torch.empty_like(x)
    lib = _lib.load()
    ws = _workspace(x.device, lib.drba_instance_norm_ws_floats(n * c))
    _lib.check(lib.drba_instance_norm(_p(x), _p(out), _p(ws), n * c, h * w, float(eps), 1 if relu else 0, _stream()),
               "drba_instance_norm")
    return out


def add_act(a, b, relu=False):
    a, b = _f32(a), _f32(b)
    assert a.shape == b.shape
    out = torch.empty_like(a)
    _lib.check(_lib.load().drba_add_act(_p(a), _p(b), _p(out), a.numel(), 1 if relu else 0, _stream()), "drba_add_act")
    return out


def channel_normalize3(x, mean, std):
    x = _f32(x)
    n, c, h, w = x.shape
    assert c == 3
    out = torch.empty_like(x)
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    _lib.check(_lib.load().drba_channel_normalize3(_p(x), _p(out), n, h * w, C.cast(m, C.c_void_p), C.cast(s, C.c_void_p),
                                                   _stream()), "drba_channel_normalize3")
    return out


def layernorm(x, w, b, residual=None, eps=1e-5):
    x = _f32(x)
    cols = x.shape[-1]
    rows = x.numel() // cols
    out = torch.empty_like(x)
    res = None if residual is None else _f32(residual)
    _lib.check(_lib.load().drba_layernorm(_p(x), _p(w), _p(b), _p(res), _p(out), rows, cols, float(eps), _stream()),
               "drba_layernorm")
    return out


def gelu(x):
    x = _f32(x)
    out = torch.empty_like(x)
    _lib.check(_lib.load().drba_gelu(_p(x), _p(out), x.numel(), _stream()), "drba_gelu")
    return out


class LinearSplit:
    """nn.Linear on token-major activations ([..., K] -> [..., N]) through drba_linear_split; optional fused GELU."""

    def __init__(self, weight, bias=None, gelu=False, device=None, terms=None):
        """terms: 3 = three bf16 terms per operand, 2 = two fp16 terms (kernel family 4); default: 2 while CONV_FAMILIES
        allows family 4."""
        self._w = weight.detach().float().cpu().contiguous()
        self.n, self.k = self._w.shape
        self.two_term_ok = two_term_ok(self._w)  # False: three bf16 terms whatever CONV_FAMILIES says
        self._terms_arg = None if terms is None else int(terms)
        self._device, self._packs = device, {}
        if _lib.load().drba_linear_split_packed_floats(self.k, self.n, self.terms) == 0:
            raise _lib.DrbaHipError(f"drba_linear_split needs K % 32 == 0 (K={self.k}) and terms in (2, 3)")
        self.bias = None if bias is None else bias.detach().float().to(device).contiguous()
        self.gelu = 1 if gelu else 0

    @property
    def terms(self):
        """Resolved at every call (ops.set_precision may change the family set while the object lives)."""
        return self._terms_arg if self._terms_arg is not None else (2 if _two_term(None, self.two_term_ok) else 3)

    @property
    def packed(self):
        t = self.terms
        if t not in self._packs:  # packed once per term count on first use
            lib = _lib.load()
            self._packs[t] = _pack_once(lib.drba_linear_split_packed_floats(self.k, self.n, t), lambda dst: lib.drba_linear_split_pack(
                C.c_void_p(self._w.data_ptr()), dst, self.k, self.n, t), "drba_linear_split_pack", self._device)
        return self._packs[t]

    @staticmethod
    def _rows(x, k):
        """x [..., k] as rows [M, k] the kernels can read in place (`k`: the layer's input width, or one part of it in cat)."""
        assert x.shape[-1] == k
        x2 = x.reshape(-1, k)  # a view for contiguous inputs and for row-strided column slices
        if x2.dtype != torch.float32 or x2.stride(1) != 1 or x2.stride(0) % 4 or x2.data_ptr() % 16 or not x2.is_cuda:
            x2 = _f32(x2)
        return x2

    def __call__(self, x):
        lead, x2 = x.shape[:-1], self._rows(x, self.k)
        m = x2.shape[0]
        out = torch.empty((m, self.n), dtype=torch.float32, device=x2.device)
        _lib.check(_timed("linear_split", (m, self.k, self.n, self.gelu), 2.0 * m * self.k * self.n, "flop", lambda: _lib.load().drba_linear_split(
            _p(x2), _p(self.packed), _p(self.bias), _p(out), m, self.k, self.n, x2.stride(0), self.gelu, self.terms, _stream())), "drba_linear_split")
        return out.view(*lead, self.n)

    def cat(self, x1, x2):
        """self(torch.cat((x1, x2), -1)) without the concatenation: the kernel reads the first K1 features of a row from
        x1 and the rest from x2."""
        k1, k2 = x1.shape[-1], x2.shape[-1]
        assert k1 + k2 == self.k and x1.shape[:-1] == x2.shape[:-1]
        lead = x1.shape[:-1]
        a, b = self._rows(x1, k1), self._rows(x2, k2)
        m = a.shape[0]
        out = torch.empty((m, self.n), dtype=torch.float32, device=a.device)
        _lib.check(_timed("linear_split_cat", (m, k1, k2, self.n, self.gelu), 2.0 * m * (k1 + k2) * self.n, "flop",
                          lambda: _lib.load().drba_linear_split_cat(_p(a), _p(b), _p(self.packed), _p(self.bias), _p(out), m, k1, k2, self.n,
                                                                    a.stride(0), b.stride(0), self.gelu, self.terms, _stream())), "drba_linear_split_cat")
        return out.view(*lead, self.n)

    def layernorm(self, x, ln_w, ln_b, residual=None, eps=1e-5):
        """residual + LayerNorm(self(x)) * ln_w + ln_b in the GEMM's epilogue (128 output features only)."""
        assert self.n == 128 and not self.gelu
        lead, x2 = x.shape[:-1], self._rows(x, self.k)
        m = x2.shape[0]
        res = None if residual is None else _f32(residual)
        out = torch.empty((m, 128), dtype=torch.float32, device=x2.device)
        lw, lb = _f32(ln_w), _f32(ln_b)
        _lib.check(_timed("linear_split_layernorm", (m, self.k, 128), 2.0 * m * self.k * 128, "flop",
                          lambda: _lib.load().drba_linear_split_layernorm(_p(x2), _p(self.packed), _p(self.bias), _p(lw), _p(lb),
                                                                          _p(res), _p(out), m, self.k, x2.stride(0), float(eps), self.terms, _stream())),
                   "drba_linear_split_layernorm")
        return out.view(*lead, 128)


ATTN_TWO_TERM = None  # None: follow CONV_FAMILIES (family 4 allowed -> the two-term fp16 kernel); True / False force it (tests, A/B)


def window_attention(q, k, v, h, w, splits, shift, scale, terms=None):
    """single_head_split_window_attention (transformer.py:46-113) fused: q, k, v [B, h*w, 128] -> [B, h*w, 128].
    q, k, v may be last-dim slices of a wider tensor (a fused projection output): only the row stride is used.
    terms: 3 = fp32 MFMA, 2 = the GEMM operands as two fp16 terms (default: 2 when kernel family 4 is allowed)."""
    if terms is None:
        terms = 2 if _two_term(ATTN_TWO_TERM) else 3
    b, n, c = q.shape
    assert n == h * w and k.shape == q.shape and v.shape == q.shape

    def rows(t):  # fp32 on the device, unit stride along channels, one constant stride between consecutive tokens
        sliced_ok = (t.dtype == torch.float32 and t.stride(2) == 1 and t.stride(0) == n * t.stride(1)
                     and t.stride(1) % 4 == 0 and t.data_ptr() % 16 == 0 and t.is_cuda)
        if t.is_contiguous() or not sliced_ok:
            t = _f32(t)  # no copy for a contiguous fp32 device tensor; raises for a CPU tensor
        return t, t.stride(1)

    (q, ldq), (k, ldk), (v, ldv) = rows(q), rows(k), rows(v)
    out = torch.empty((b, n, c), dtype=torch.float32, device=q.device)
    lib = _lib.load()
    nws = lib.drba_window_attention_ws_floats(b, h, w, int(splits))
    ws = _workspace(q.device, nws) if nws else None
    # QK^T and PV: 2 x 2 L^2 C FLOP per window of L = (h / splits)(w / splits) tokens, b * splits^2 windows
    L = (h // int(splits)) * (w // int(splits))
    _lib.check(_timed("window_attention", (b, h, w, c, int(splits), int(bool(shift)), int(terms)), 4.0 * b * int(splits) ** 2 * L * L * c, "flop",
                      lambda: lib.drba_window_attention(_p(q), _p(k), _p(v), _p(out), b, h, w, c, int(splits), int(bool(shift)),
                                                        float(scale), ldq, ldk, ldv, _p(ws), int(terms), _stream())), "drba_window_attention")
    return out


def softmax_rows_(scores, scale, mask=None):
    """In-place softmax over the last dim of scores [M, L, cols] / scale (+ mask [n_masks, L, cols] cycled over M)."""
    assert scores.is_contiguous() and scores.dtype == torch.float32
    cols = scores.shape[-1]
    rows_per_mat = scores.shape[-2]
    rows = scores.numel() // cols
    n_masks = 1
    if mask is not None:
        mask = _f32(mask)
        n_masks = mask.shape[0]
    _lib.check(_lib.load().drba_softmax_rows(_p(scores), _p(mask), rows, cols, rows_per_mat, n_masks, float(scale),
                                             _stream()), "drba_softmax_rows")
    return scores


def global_expect2(q_tok, k_tok, vals, w, scale):
    """softmax(q k^T / scale) . vals without the score matrix: q_tok, k_tok [L, 128] token-major (row-strided column
    slices allowed), vals None (pixel coordinates, own coordinate subtracted: the correlation flow) or [2, L] -> [2, L]."""
    def rows(t):
        ok = (t.dim() == 2 and t.dtype == torch.float32 and t.is_cuda and t.stride(1) == 1 and t.stride(0) % 4 == 0
              and t.data_ptr() % 16 == 0)
        t = t if ok else _f32(t.reshape(-1, t.shape[-1]))
        return t, t.stride(0)
    (q, ldq), (k, ldk) = rows(q_tok), rows(k_tok)
    L, c = q.shape
    assert k.shape == (L, c)
    v = None if vals is None else _f32(vals)
    if v is not None:
        assert v.numel() == 2 * L
    out = torch.empty((2, L), dtype=torch.float32, device=q.device)
    lib = _lib.load()
    nws = lib.drba_global_expect2_ws_floats(L)
    ws = _workspace(q.device, nws) if nws else None
    _lib.check(_timed("global_expect2", (L, c), 2.0 * L * L * c, "flop", lambda: lib.drba_global_expect2(
        _p(q), _p(k), _p(v), _p(out), _p(ws), L, c, int(w), float(scale), ldq, ldk, _stream())), "drba_global_expect2")
    return out


def bmm(a, b, trans_b):
    """[B, M, K] x ([B, N, K]^T if trans_b else [B, K, N]) -> [B, M, N]; plain fp32 kernel for the degenerate attention case."""
    a, b = _f32(a), _f32(b)
    bsz, m, kk = a.shape
    n = b.shape[1] if trans_b else b.shape[2]
    out = torch.empty((bsz, m, n), dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().drba_bmm(_p(a), _p(b), _p(out), bsz, m, n, kk, 1 if trans_b else 0, _stream()), "drba_bmm")
    return out


def local_corr_flow(f0, f1, radius):
    f0, f1 = _f32(f0), _f32(f1)
    n, c, h, w = f0.shape
    assert n == 1
    out = torch.empty((1, 2, h, w), dtype=torch.float32, device=f0.device)
    _lib.check(_lib.load().drba_local_corr_flow(_p(f0), _p(f1), _p(out), c, h, w, int(radius), _stream()),
               "drba_local_corr_flow")
    return out


def local_attn_flow(q_tok, k_tok, flow, radius):
    q_tok, k_tok, flow = _f32(q_tok), _f32(k_tok), _f32(flow)
    _, _, h, w = flow.shape
    c = q_tok.shape[-1]
    out = torch.empty_like(flow)
    _lib.check(_lib.load().drba_local_attn_flow(_p(q_tok), _p(k_tok), _p(flow), _p(out), c, h, w, int(radius), _stream()),
               "drba_local_attn_flow")
    return out


def convex_upsample(mask, flow, factor):
    mask, flow = _f32(mask), _f32(flow)
    _, _, h, w = flow.shape
    out = torch.empty((1, 2, factor * h, factor * w), dtype=torch.float32, device=flow.device)
    _lib.check(_lib.load().drba_convex_upsample(_p(mask), _p(flow), _p(out), h, w, int(factor), _stream()),
               "drba_convex_upsample")
    return out


def flow_warp(x, flow):
    x, flow = _f32(x), _f32(flow)
    n, c, h, w = x.shape
    assert n == 1
    out = torch.empty_like(x)
    _lib.check(_lib.load().drba_flow_warp(_p(x), _p(flow), _p(out), c, h, w, _stream()), "drba_flow_warp")
    return out


def resize_bilinear_ac(x, size, mul=1.0):
    x = _f32(x)
    n, c, h, w = x.shape
    out = torch.empty((n, c, int(size[0]), int(size[1])), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().drba_resize_bilinear_ac(_p(x), _p(out), n * c, h, w, int(size[0]), int(size[1]), float(mul),
                                                   _stream()), "drba_resize_bilinear_ac")
    return out
