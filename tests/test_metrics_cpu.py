"""CPU (-m "not gpu"): the host side of the picture metrics (drba_amd.metrics, drba_amd.evaluate) and the checks themselves.

  * the new entry points of the library validate their arguments before any launch;
  * the rows of tests/metric_checks.py pass for a correct stand-in and FAIL for the defects they are there for: an SSIM
    without the channel pass, with zero padding, the fp32 cancelling formula on flat content, a 32-bit error accumulator;
  * the hold-out procedure pairs every emission with the right original frame (a recording fake model, a numpy back end);
  * compare: gates, exit codes, the JSON object, mismatched clips; ClipMetrics' summary arithmetic on planted values."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

from drba_amd import _lib, evaluate, metrics
from tests import metric_checks as mc


def _failed(rows):
    return [r[0] for r in rows if not r[1] <= r[2]]


# ----------------------------------------------------------------------------------------------------------- entry points
def test_metric_entry_points_validate_arguments_without_gpu():
    lib = _lib.load()
    buf = torch.zeros(4096)
    p = C.c_void_p(buf.data_ptr())
    assert lib.drba_ssim3d(None, p, p, p, 1, 16, 16, 0, 0.0, None) == -1
    assert lib.drba_ssim3d(p, None, p, p, 1, 16, 16, 0, 0.0, None) == -1
    assert lib.drba_ssim3d(p, p, None, p, 1, 16, 16, 0, 0.0, None) == -1
    assert lib.drba_ssim3d(p, p, p, None, 1, 16, 16, 0, 0.0, None) == -1
    assert lib.drba_ssim3d(p, p, p, p, 0, 16, 16, 0, 0.0, None) == -1
    assert lib.drba_ssim3d(p, p, p, p, 1, 16, 16, 2, 0.0, None) == -1          # unknown dtype
    assert lib.drba_ssim3d(p, p, p, p, 1, 16, 16, 0, -1.0, None) == -1         # negative range
    assert lib.drba_ssim3d(p, p, p, p, 1, 16, 16, 0, float("nan"), None) == -1
    for h, w in ((10, 16), (16, 10), (1, 1)):
        assert lib.drba_ssim3d(p, p, p, p, 1, h, w, 0, 0.0, None) == -2          # the reference shrinks its window there
        assert lib.drba_ssim3d(p, p, p, p, 1, h, w, 1, 1.0, None) == -2
    for fn in (lib.drba_frame_error_u8, lib.drba_frame_error_f32):
        assert fn(None, p, p, p, 1, 16, None) == -1
        assert fn(p, None, p, p, 1, 16, None) == -1
        assert fn(p, p, None, p, 1, 16, None) == -1
        assert fn(p, p, p, None, 1, 16, None) == -1
        assert fn(p, p, p, p, 0, 16, None) == -1
        assert fn(p, p, p, p, 1, 0, None) == -1
    # workspaces: tile sums (doubles) + range partials for SSIM, 512 partial results of 32 bytes per item for the differences
    assert lib.drba_ssim3d_ws_floats(2, 17, 33) == 2 * 4 * 2 + 2 * 256 * 2
    assert lib.drba_ssim3d_ws_floats(1, 2160, 3840) == 120 * 135 * 2 + 512
    assert lib.drba_ssim3d_ws_floats(0, 16, 16) == 0
    assert lib.drba_frame_error_ws_floats(3, 1) == 3 * 512 * 8 and lib.drba_frame_error_ws_floats(0, 5) == 0


def test_metrics_have_no_cpu_fallback():
    if not torch.cuda.is_available():
        with pytest.raises(_lib.DrbaHipError):
            metrics.ssim(np.zeros((16, 16, 3), np.uint8), np.zeros((16, 16, 3), np.uint8))


# ------------------------------------------------------------------------------------------------------ rows discriminate
def test_truth_agrees_with_the_fp32_oracle_where_the_oracle_can_be_trusted():
    """On noise the fp32 formula does not cancel: the oracle (bit-equal to the reference) and the float64 truth agree to fp32
    roundoff -- the truth restates the same definition.  On the flat pair the oracle misses the bar the kernel is held to."""
    for name, a, b, vr, truth, ora in mc.ssim_cases():
        if ora is None:
            continue
        err = float(np.abs(ora - truth).max())
        if name.endswith(" noise"):
            assert err < 5e-6, (name, err)
        if name.endswith(" flat"):
            assert err > 4 * mc.SSIM_TOL, (name, err)


def test_folded_dense_blur_equals_the_volume_convolution():
    """the form of the truth used on large frames against the plain conv3d form, on every kind of input"""
    for a, b in (mc.noise_pair(45, 70, 9), mc.flat_pair(17, 33), mc.synth_pair(13, 37), mc.noise_pair(11, 11, 9, -1.0, 1.0)):
        x, y = a.double().unsqueeze(1), b.double().unsqueeze(1)
        f = torch.cat([x, y, x * x, y * y, x * y])
        assert float((mc.blur_dense(f) - mc.blur_dense_folded(f)).abs().max()) <= 1e-13
        assert abs(mc.ssim_truth(a, b, blur=mc.blur_dense)[0] - mc.ssim_truth(a, b, blur=mc.blur_dense_folded)[0]) <= 1e-12


def test_ssim_rows_pass_for_the_definition_and_fail_for_each_defect():
    good = mc.check_ssim(lambda a, b, vr: mc.ssim_separable64(a, b, vr))
    assert not _failed(good), _failed(good)
    assert len(good) >= 3 * len(mc.SSIM_SHAPES) + 5
    no_mix = _failed(mc.check_ssim(lambda a, b, vr: mc.ssim_separable64(a, b, vr, channel_mix=False)))
    assert any("synth" in n for n in no_mix) and any("noise" in n for n in no_mix), no_mix
    zero_pad = _failed(mc.check_ssim(lambda a, b, vr: mc.ssim_separable64(a, b, vr, replicate=False)))
    assert any("11x11" in n for n in zero_pad) and any("270x480" in n for n in zero_pad), zero_pad
    fp32 = _failed(mc.check_ssim(lambda a, b, vr: mc.ssim_oracle32(a, b) if not vr else mc.ssim_separable64(a, b, vr)))
    flat = [r[0] for r in good if r[0].endswith(" flat")]
    assert len(flat) == len(mc.SSIM_SHAPES) and set(flat) <= set(fp32), fp32  # every flat row catches the cancelling formula


def test_error_rows_pass_for_exact_sums_and_fail_for_a_32_bit_accumulator():
    def exact(a, b, N, n, oa, ob):
        return mc.err_u8_ref(a, b, N, n)

    def acc32(a, b, N, n, oa, ob):
        d = np.abs(a.astype(np.int64).reshape(N, n) - b.astype(np.int64).reshape(N, n)).astype(np.uint32)
        return np.stack([(d * d).sum(1, dtype=np.uint32), d.sum(1, dtype=np.uint32), d.max(1), (d != 0).sum(1, dtype=np.uint32)], 1)

    assert not _failed(mc.check_frame_error_u8(exact))
    bad = _failed(mc.check_frame_error_u8(acc32))
    assert bad and all("70000" in n for n in bad) and any("2^32" in n for n in bad), bad

    def f64(a, b, N, n):
        return mc.err_f32_ref(a, b, N, n)

    def f32acc(a, b, N, n):
        s, nf = mc.err_f32_ref(a, b, N, n)
        d = np.abs(a.reshape(N, n) - b.reshape(N, n))
        d = np.where(np.isfinite(d), d, np.float32(0))
        return np.stack([np.cumsum(d * d, 1, dtype=np.float32)[:, -1], np.cumsum(d, 1, dtype=np.float32)[:, -1], s[:, 2]], 1), nf

    assert not _failed(mc.check_frame_error_f32(f64))
    assert any("sums" in n for n in _failed(mc.check_frame_error_f32(f32acc)))


# ------------------------------------------------------------------------------------------------------------ ClipMetrics
def test_summary_arithmetic_on_planted_values():
    mse = [0.0, 4.0, 1.0, 0.0, 4.0]
    ssim = [1.0, 0.7, 0.9, 1.0, 0.6]
    s = metrics.summarise(mse, ssim, [0, 9, 2, 0, 5], [0, 120, 30, 0, 77], peak=255.0)
    pf, sm = s["per_frame"], s["summary"]
    p4, p1 = 10 * math.log10(255.0 ** 2 / 4.0), 10 * math.log10(255.0 ** 2)
    assert pf["psnr"] == [math.inf, p4, p1, math.inf, p4]
    assert sm["mean_psnr"] == pytest.approx((2 * p4 + p1) / 3, rel=1e-15)              # over the finite ones
    assert sm["psnr_of_mean_mse"] == pytest.approx(10 * math.log10(255.0 ** 2 / 1.8), rel=1e-15)
    assert sm["mean_ssim"] == pytest.approx(0.84) and sm["min_ssim"] == 0.6
    assert sm["max_lsb"] == 9 and sm["total_differing"] == 227
    assert sm["worst_frame"] == 4                                                       # lowest PSNR, the tie broken by SSIM
    same = metrics.summarise([0.0, 0.0], [1.0, 1.0], [0, 0], [0, 0], peak=255.0)["summary"]
    assert same["mean_psnr"] == math.inf and same["psnr_of_mean_mse"] == math.inf and same["worst_frame"] == 0
    empty = metrics.summarise([], [], [], [], peak=255.0)
    assert empty["frames"] == 0 and empty["summary"]["worst_frame"] is None


def test_clip_metrics_over_an_injected_back_end():
    be = mc.NumpyBackend()
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (5, 16, 24, 3), dtype=np.uint8)
    b = a.copy()
    b[1, 2, 3, 1] ^= 4
    b[3, :4] = 255 - b[3, :4]
    cm = metrics.ClipMetrics(backend=be, capacity=2)  # three chunks of slots
    for k in range(3):
        cm.add(a[k], b[k])
    cm.add(a[3:], b[3:])  # two frames in one call
    assert len(cm) == 5
    r = cm.result()
    d = np.abs(a.astype(np.int64) - b.astype(np.int64)).reshape(5, -1)
    assert r["per_frame"]["differing"] == (d != 0).sum(1).tolist() and r["per_frame"]["max_lsb"] == d.max(1).tolist()
    mse = (d * d).mean(1)
    assert r["per_frame"]["psnr"] == [metrics.psnr_of_mse(v, 255.0) for v in mse]
    assert r["per_frame"]["ssim"][0] == 1.0 and r["per_frame"]["ssim"][3] < 0.9
    assert r["summary"]["worst_frame"] == 3 and r["summary"]["total_differing"] == int((d != 0).sum())
    # the one-shot functions over the same back end
    assert metrics.psnr(a[1], b[1], backend=be) == metrics.psnr_of_mse(mse[1], 255.0)
    assert metrics.psnr(a[0], b[0], backend=be) == math.inf
    assert metrics.frame_error(a[3], b[3], backend=be) == {"sum_sq": int((d[3] ** 2).sum()), "sum_abs": int(d[3].sum()), "max_abs": int(d[3].max()),
                                                          "differing": int((d[3] != 0).sum()), "n": 16 * 24 * 3}
    assert metrics.ssim(a[2], b[2], backend=be) == 1.0
    with pytest.raises(ValueError):
        cm.add(a[0], a[0, :8])


# --------------------------------------------------------------------------------------------------------------- hold-out
class _LinearModel:
    """Frames are constant images whose value is the position on the kept-frame axis times 16: an interpolation at t between
    values v0, v1 is v0 + t (v1 - v0).  Records every call."""
    scale, pad_size = 1.0, 1

    def __init__(self):
        self.calls = []

    def inference_ts(self, I0, I1, ts):
        self.calls.append(("ts", [float(t) for t in ts]))
        return [I0 + float(t) * (I1 - I0) for t in ts]

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False, **kw):
        self.calls.append(("drba", [float(t) for t in ts]))
        return [I0 + float(t) * (I1 - I0) if t < 1 else I1 + (float(t) - 1) * (I2 - I1) for t in ts], None


def _ramp_clip(n, k, h=12, w=14):
    """original frame p is the constant image of value round(p * 48 / k): on the kept-frame axis 48 per step"""
    return np.stack([np.full((h, w, 3), round(p * 48 / k) % 256, np.uint8) for p in range(n)])


def _hooks():
    to_inp = lambda fr, size: torch.from_numpy(np.ascontiguousarray(fr)).float()  # noqa: E731
    to_out = lambda x, size: np.rint(x.numpy()).astype(np.uint8)  # noqa: E731
    return to_inp, to_out


@pytest.mark.parametrize("k,m", [(3, 2), (3, 4), (5, 2), (5, 4)])
@pytest.mark.parametrize("plain", [False, True])
def test_holdout_pairs_every_emission_with_its_original(k, m, plain):
    n = m * k + 1 + (k - 1)  # the frames past m k + 1 are not used
    frames = _ramp_clip(n, k)
    model, be = _LinearModel(), mc.NumpyBackend()
    to_inp, to_out = _hooks()
    res = evaluate.holdout(model, frames, k, plain=plain, backend=be, to_inp=to_inp, to_out=to_out)
    half = (k - 1) // 2
    assert res["emissions"] == k * (m + 1) and res["frames_used"] == m * k + 1 and res["m"] == m
    assert res["pairs"] == [(j, j - half) for j in range(half, k * (m + 1) - half)]  # the 2 * half end copies are left out
    assert res["kept"]["positions"] == [i * k for i in range(m + 1)]
    assert res["held_out"]["positions"] == [p for p in range(m * k + 1) if p % k]
    assert res["kept"]["frames"] == m + 1 and res["held_out"]["frames"] == m * (k - 1)
    # every compared pair is (emission, the original at its position): the back end saw exactly the originals ...
    for (j, p), (got, orig) in zip(res["pairs"], be.pairs):
        assert np.array_equal(orig, frames[p]), (j, p)
    # ... and a linear model on a linear ramp reproduces them (to the rounding of the ramp itself): a shifted pairing would not
    assert res["kept"]["summary"]["max_lsb"] == 0 and res["held_out"]["summary"]["max_lsb"] <= 1
    assert res["held_out"]["summary"]["mean_ssim"] > 0.99
    kinds = {c[0] for c in model.calls}
    assert kinds == ({"ts"} if plain else {"ts", "drba"})
    rep = evaluate.holdout_report(res)
    json.dumps(evaluate._jsonable(rep))
    assert rep["kept"]["frames"] == m + 1 and rep["held_out"]["positions"] == res["held_out"]["positions"]


def test_holdout_figures_move_when_the_held_out_frames_are_one_position_off():
    """the check above is able to fail: with every held-out original replaced by its successor the kept frames still agree
    and the held-out ones are a whole step (16) away"""
    k, m = 3, 2
    frames = _ramp_clip(m * k + 1, k)
    off = frames.copy()
    for p in range(m * k):
        if p % k:
            off[p] = frames[p + 1]
    to_inp, to_out = _hooks()
    res = evaluate.holdout(_LinearModel(), off, k, backend=mc.NumpyBackend(), to_inp=to_inp, to_out=to_out)
    assert res["kept"]["summary"]["max_lsb"] == 0 and res["held_out"]["summary"]["max_lsb"] == 16


@pytest.mark.parametrize("k,n,word", [(4, 20, "even"), (2, 20, "at least 3"), (1, 20, "at least 3"), (3, 6, "at least 7 frames"),
                                      (5, 10, "at least 11 frames")])
def test_holdout_refuses_what_it_cannot_align(k, n, word):
    with pytest.raises(ValueError, match=word):
        evaluate.holdout_plan(n, k)
    with pytest.raises(ValueError, match=word):
        evaluate.holdout(_LinearModel(), _ramp_clip(n, max(k, 1)), k, backend=mc.NumpyBackend(), to_inp=_hooks()[0], to_out=_hooks()[1])
    assert evaluate.holdout_plan(7, 3) == (2, 1) and evaluate.holdout_plan(21, 5) == (4, 2)


# ---------------------------------------------------------------------------------------------------------------- compare
def _two_clips(tmp_path):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (4, 16, 20, 3), dtype=np.uint8)
    b = a.copy()
    b[1, 0, 0, 0] = a[1, 0, 0, 0] ^ 1          # 1 LSB in one byte
    b[2, 5:9, 3:7] = 255 - a[2, 5:9, 3:7]      # a block inverted
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npy")
    np.savez(pa, frames=a, fps=np.float64(30.0))
    np.save(pb, b)
    json.dump({"fps": 30.0}, open(str(tmp_path / "b.json"), "w"))
    return a, b, pa, pb


def test_compare_report_gates_and_exit_codes(tmp_path, capsys):
    a, b, pa, pb = _two_clips(tmp_path)
    be = mc.NumpyBackend()
    out_json = str(tmp_path / "rep.json")
    assert evaluate.main(["compare", pa, pb, "--json", out_json], backend=be) == 0      # no gate given
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    d = np.abs(a.astype(np.int64) - b.astype(np.int64)).reshape(4, -1)
    mse = (d * d).mean(1)
    psnr = [metrics.psnr_of_mse(v, 255.0) for v in mse]
    assert rep["command"] == "compare" and rep["frames"] == 4 and rep["size"] == [16, 20] and rep["ok"] is True and rep["gates"] == {}
    assert rep["max_lsb"] == int(d.max()) and rep["total_differing"] == int((d != 0).sum()) and rep["worst_frame"] == 2
    assert rep["min_psnr"] == pytest.approx(min(psnr)) and rep["mean_psnr"] == pytest.approx(np.mean([p for p in psnr if math.isfinite(p)]))
    assert rep["psnr_of_mean_mse"] == pytest.approx(metrics.psnr_of_mse(mse.mean(), 255.0))
    assert set(rep) == {"command", "a", "b", "frames", "size", "peak", "mean_psnr", "psnr_of_mean_mse", "mean_ssim", "min_ssim",
                        "max_lsb", "total_differing", "worst_frame", "min_psnr", "gates", "ok"}
    full = json.load(open(out_json))
    assert [float(v) for v in full["per_frame"]["psnr"]] == psnr and full["per_frame"]["psnr"][0] == "inf"
    assert full["per_frame"]["differing"] == (d != 0).sum(1).tolist()
    # gates that hold: exit 0; each gate violated on its own: exit 1, and the report names it
    lo_ssim = rep["min_ssim"]
    assert evaluate.main(["compare", pa, pb, "--max-lsb", "255", "--min-psnr", "1", "--min-ssim", "-1"], backend=be) == 0
    for argv, gate in ((["--max-lsb", "1"], "max_lsb"), (["--min-psnr", str(min(psnr) + 1)], "min_psnr"), (["--min-ssim", str(lo_ssim + 0.01)], "min_ssim")):
        capsys.readouterr()
        assert evaluate.main(["compare", pa, pb] + argv, backend=be) == 1, argv
        r = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert r["ok"] is False and r["gates"][gate]["ok"] is False and list(r["gates"]) == [gate]
    # a clip against itself passes the strictest gates
    assert evaluate.main(["compare", pa, pa, "--max-lsb", "0", "--min-ssim", "1", "--min-psnr", "200"], backend=be) == 0
    r = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert r["mean_psnr"] == "inf" and r["max_lsb"] == 0 and r["min_ssim"] == 1.0


def test_compare_refuses_mismatched_clips(tmp_path, capsys):
    a, b, pa, pb = _two_clips(tmp_path)
    short, small = str(tmp_path / "short.npz"), str(tmp_path / "small.npz")
    np.savez(short, frames=a[:3])
    np.savez(small, frames=a[:, :12])
    be = mc.NumpyBackend()
    assert evaluate.main(["compare", pa, short], backend=be) == 2
    err = capsys.readouterr().err
    assert "4 frames against 3" in err
    assert evaluate.main(["compare", pa, small], backend=be) == 2
    err = capsys.readouterr().err
    assert "(16, 20) against (12, 20)" in err
    assert evaluate.main(["compare", pa, str(tmp_path / "missing.npz")], backend=be) == 2
    with pytest.raises(ValueError, match="3 frames against 2"):  # sources without a length (containers) are counted as they are read
        evaluate.compare(iter(list(a[:3])), iter(list(a[:2])), backend=be)
