"""CPU: the non-linear DRBA mode outside the kernels -- the host walk of get_drm_t's bisection (drba_drm_walk) against the
reference's loop, the --nonlinear switches of infer.py and of the hold-out command, and the driver loop handing `linear` to
every inference_ts_drba call."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from drba_amd import _lib, evaluate
from drba_amd import infer as drv
from tests import metric_checks as mc


# ------------------------------------------------------------------------------------------------------------- the walk
def reference_walk(t, precision):
    """The scalar part of the reference's get_drm_t (models/drm.py:36-37, :43-56), literally -> 'D' for each `_x > t` update,
    'U' for each `_x < t` update, in order; None once it has made more than 64 of them."""
    _x, b = 0.5, 0.5
    l, r = 0, 1
    moves = []
    while abs(_x - t) > precision:
        if _x > t:
            r = _x
            _x = _x - (_x - l) * b
            moves.append("D")
        if _x < t:
            l = _x
            _x = _x + (r - _x) * b
            moves.append("U")
        if len(moves) > 64:
            return None
    return "".join(moves)


def library_walk(t, precision):
    moves, n = C.c_uint32(), C.c_int()
    rc = _lib.load().drba_drm_walk(float(t), float(precision), C.byref(moves), C.byref(n))
    if rc != 0:
        return rc
    assert 0 <= n.value <= 32 and (n.value == 32 or moves.value >> n.value == 0)  # no bit beyond the count
    return "".join("U" if (moves.value >> k) & 1 else "D" for k in range(n.value))


TS = (0.5, 0.5005, 0.25, 0.75, 0.1, 0.9, 0.4, 0.6, 0.3, 0.7, 1 / 3, 0.001, 0.999, 0.0005)


@pytest.mark.parametrize("precision", [1e-3, 5e-2, 1e-5])
@pytest.mark.parametrize("t", TS)
def test_walk_equals_the_reference_loop(t, precision):
    want = reference_walk(t, precision)
    assert want is not None and len(want) <= 32
    assert library_walk(t, precision) == want


def test_walk_facts_at_the_model_precision():
    """What the kernel's cost rests on: no move at t = 0.5 (u = r), one at the quarters, 8 or 9 elsewhere; both updates can fire
    in one iteration (t = 1/3: four iterations, eight moves)."""
    n = {t: len(library_walk(t, 1e-3)) for t in TS}
    assert n[0.5] == 0 and n[0.5005] == 0 and n[0.25] == 1 and n[0.75] == 1
    assert all(n[t] == 8 for t in (0.1, 0.4, 0.6, 0.9, 1 / 3, 0.001, 0.999)) and n[0.0005] == 9
    assert library_walk(1 / 3, 1e-3) == "DUDUDUDU"
    assert max(n.values()) <= 9


def test_walk_longer_than_the_mask_is_unsupported_and_bad_arguments_are_refused():
    lib = _lib.load()
    assert len(reference_walk(0.3, 1e-12) or "x" * 65) > 32
    assert library_walk(0.3, 1e-12) == -2          # DRBA_EUNSUPPORTED: ops then runs the composition
    assert library_walk(2.0, 1e-3) == -2           # a t the bisection never reaches
    m, n = C.c_uint32(), C.c_int()
    assert lib.drba_drm_walk(0.3, 0.0, C.byref(m), C.byref(n)) == -1
    assert lib.drba_drm_walk(0.3, 1e-3, None, C.byref(n)) == -1 and lib.drba_drm_walk(0.3, 1e-3, C.byref(m), None) == -1
    # the two kernel entry points validate like the linear ones, before any launch
    assert lib.drba_drm_rife_nonlinear(None, None, 0.3, 1e-3, 1e-4, None, None, 1, 8, 8, None) == -1
    assert lib.drba_drm_rife_nonlinear_batch(None, 1, 1e-3, 1e-4, None, 8, 8, None) == -1
    jobs = (_lib.DrmNonlinearJob * 9)()
    assert lib.drba_drm_rife_nonlinear_batch(C.cast(jobs, C.c_void_p), 9, 1e-3, 1e-4, C.c_void_p(8), 8, 8, None) == -1  # > DRBA_MAX_STAGE_ITEMS
    assert lib.drba_drm_rife_nonlinear_batch(C.cast(jobs, C.c_void_p), 2, 1e-3, 1e-4, C.c_void_p(8), 8, 8, None) == -1  # null tensors in a job


# ------------------------------------------------------------------------------------------------------------- command line
def test_parse_args_nonlinear_defaults_off_and_changes_nothing_else():
    a = drv.parse_args([])
    assert a.nonlinear is False and a.out_depth == "source"
    assert (a.model_type, a.input, a.output, a.dst_fps, a.times, a.enable_scdet, a.scdet_threshold, a.hwaccel, a.scale) == \
        ("rife", "input.mp4", "output.mp4", 60, -1, False, 0.3, False, 1.0)
    b = drv.parse_args(["-m", "gmfss", "-i", "a.npz", "-o", "b.npz", "-t", "2", "-s", "-st", "0.2", "-hw", "-scale", "0.5", "--nonlinear"])
    assert b.nonlinear is True and b.out_depth == "source"
    assert (b.model_type, b.input, b.output, b.times, b.enable_scdet, b.scdet_threshold, b.hwaccel, b.scale) == \
        ("gmfss", "a.npz", "b.npz", 2, True, 0.2, True, 0.5)
    assert drv.parse_args(["--out-depth", "16"]).nonlinear is False


# ------------------------------------------------------------------------------------------------------------- driver loop
class Tagged:
    def __init__(self, kind, ident):
        self.kind, self.ident = kind, ident


class FakeIO:
    def __init__(self, frames, fps):
        self.src_fps, self.total_frames_count = fps, len(frames)
        self._it = iter(list(frames) + [None])
        self.written = []

    def read_frame(self):
        return next(self._it)

    def write_frame(self, x):
        self.written.append(x)


class FakeModel:
    """Records every call; takes no lookahead (the plain reference surface)."""

    def __init__(self):
        self.scale, self.pad_size = 1.0, 64
        self.log, self.n_gen = [], 0

    def _gen(self):
        self.n_gen += 1
        return Tagged("gen", self.n_gen)

    def inference_ts(self, I0, I1, ts):
        self.log.append(["ts", I0.ident, I1.ident, [float(t) for t in ts]])
        return [I0 if t == 0 else I1 if t == 1 else self._gen() for t in ts]

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False):
        self.log.append(["drba", I0.ident, I1.ident, I2.ident, [float(t) for t in ts], reuse is None, linear])
        return [I0 if t == 0 else I1 if t == 1 else I2 if t == 2 else self._gen() for t in ts], ("reuse", I2.ident)


class LookaheadModel(FakeModel):
    supports_lookahead = True

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False, lookahead=None):
        return super().inference_ts_drba(I0, I1, I2, ts, reuse, linear)


CUTS = {(5, 6), (6, 7), (10, 11)}  # frame 6 has a cut on both sides; 10 | 11 a single one


def _run(model, **kw):
    frames = [np.full((8, 8, 3), k, np.uint8) for k in range(14)]
    index = {id(f): k for k, f in enumerate(frames)}
    io = FakeIO(frames, 24.0)
    n = drv.interpolate_stream(model, io, 60.0, enable_scdet=True, to_inp=lambda fr, size: Tagged("copy", index[id(fr)]),
                               to_out=lambda x, size: (x.kind, x.ident),
                               check_scene=lambda a, b, thr: (a.ident, b.ident) in CUTS, **kw)
    assert n == len(io.written)
    return model.log, io.written


@pytest.mark.parametrize("cls", [FakeModel, LookaheadModel])
def test_driver_hands_linear_to_every_drba_call(cls):
    base_log, base_written = _run(cls())
    drba = [c for c in base_log if c[0] == "drba"]
    assert len(drba) >= 6 and any(c[0] == "ts" for c in base_log[1:-1])  # DRBA steps and the cut branches between them
    assert all(c[-1] is True for c in drba)                              # the default: the reference driver's linear=True
    for flag in (True, False):
        log, written = _run(cls(), linear=flag)
        assert all(c[-1] is flag for c in log if c[0] == "drba")
        assert [c[:-1] if c[0] == "drba" else c for c in log] == [c[:-1] if c[0] == "drba" else c for c in base_log]  # same calls, same order
        assert written == base_written                                    # same emissions


# ------------------------------------------------------------------------------------------------------------- hold-out
class _RampModel:
    scale, pad_size = 1.0, 1

    def __init__(self):
        self.linear = []

    def inference_ts(self, I0, I1, ts):
        return [I0 + float(t) * (I1 - I0) for t in ts]

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False, **kw):
        self.linear.append(linear)
        return [I0 + float(t) * (I1 - I0) if t < 1 else I1 + (float(t) - 1) * (I2 - I1) for t in ts], None


def _ramp(n, k):
    return np.stack([np.full((12, 14, 3), round(p * 48 / k) % 256, np.uint8) for p in range(n)])


def _hooks():
    return (lambda fr, size: torch.from_numpy(np.ascontiguousarray(fr)).float(),
            lambda x, size: np.rint(x.numpy()).astype(np.uint8))


@pytest.mark.parametrize("linear", [True, False])
def test_holdout_runs_in_the_mode_asked_for_and_reports_it(linear):
    to_inp, to_out = _hooks()
    model = _RampModel()
    res = evaluate.holdout(model, _ramp(7, 3), 3, backend=mc.NumpyBackend(), to_inp=to_inp, to_out=to_out, linear=linear)
    assert model.linear and all(v is linear for v in model.linear)
    rep = evaluate.holdout_report(res)
    assert rep["linear"] is linear and rep["plain"] is False
    assert json.loads(json.dumps(evaluate._jsonable(rep)))["linear"] is linear
    default = evaluate.holdout_report(evaluate.holdout(_RampModel(), _ramp(7, 3), 3, backend=mc.NumpyBackend(), to_inp=to_inp, to_out=to_out))
    assert default["linear"] is True


def test_holdout_refuses_nonlinear_together_with_plain(tmp_path, capsys):
    to_inp, to_out = _hooks()
    with pytest.raises(ValueError, match="--nonlinear and --plain"):
        evaluate.holdout(_RampModel(), _ramp(7, 3), 3, plain=True, linear=False, backend=mc.NumpyBackend(), to_inp=to_inp, to_out=to_out)
    clip = str(tmp_path / "clip.npz")
    np.savez(clip, frames=_ramp(7, 3), fps=np.float64(24.0))
    a = evaluate.parse_args(["holdout", "-i", clip])
    assert a.nonlinear is False and a.plain is False
    assert evaluate.parse_args(["holdout", "-i", clip, "--nonlinear"]).nonlinear is True
    assert evaluate.main(["holdout", "-i", clip, "--nonlinear", "--plain"]) == 2  # refused before a model is loaded
    assert "--nonlinear and --plain" in capsys.readouterr().err
