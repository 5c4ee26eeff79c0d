"""GPU: --dedup on the device -- the duplicate statistic (dedup.hip: drba_dup_stats_f32) against the fp64 numpy reference of
tests/dedup_common.py, the filter's decisions on a clip with planted repeats, and the command line: the doubling identity (a clip on
twos at x2 with --dedup writes what the clip itself writes at x4), unequal gaps against the CPU oracle driver, a clip without repeats,
and a Y4M stream through stdin and stdout.  Every command line runs in ONE child process (one model load), started once per module."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from drba_amd import dedup, driver, ops, y4m
from drba_amd.models.utils import tools
from drba_amd.utils import synth
from tests import dedup_common as dc
from tests import yuv_common as yc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 96, 160


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------ statistic
@pytest.mark.parametrize("last_block", [False, True], ids=["inner_block", "last_block"])
@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dup_stats_against_fp64(dev, shape, last_block):
    """max_block within 1e-5 relative of the fp64 reference (a block sums at most 192 fp32 terms: 192 * 2^-24 = 1.1e-5 bounds the
    rounding), n_above and n_blocks equal to it -- on inputs whose reference has no block mean within 1e-4 relative of lo (asserted
    on the reference first) -- and the same bytes from a second call."""
    a, b, (by, bx) = dc.seeded_pair(*shape, last_block=last_block)
    want_max, want_above, want_blocks, margin = dc.ref_stats(a, b)
    assert margin > 1e-4, margin
    means = dc.block_means(a, b)
    assert np.unravel_index(np.argmax(means), means.shape) == (by, bx)  # the planted patch holds the maximum
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    got = ops.dup_stats(ta, tb, dc.LO)
    print(f"dup_stats {shape} last={last_block}: device {got}, fp64 {(want_max, want_above, want_blocks)}, "
          f"rel {abs(got[0] - want_max) / want_max:.2e}, margin {margin:.2e}")
    assert abs(got[0] - want_max) <= 1e-5 * want_max
    assert got[1:] == (want_above, want_blocks)
    raw = [ops._dup_stats_enqueue(ta, tb, dc.LO).cpu().numpy().tobytes() for _ in range(2)]
    assert raw[0] == raw[1]
    # a view whose base is not 16-byte aligned takes the scalar loads: the same sums
    flat = torch.empty(ta.numel() + 1, dtype=torch.float32, device=dev)
    flat[1:] = ta.reshape(-1)
    assert ops._dup_stats_enqueue(flat[1:].view_as(ta), tb, dc.LO).cpu().numpy().tobytes() == raw[0]
    assert ops.dup_stats(ta, ta, dc.LO) == (0.0, 0, want_blocks)
    host, ev = ops.dup_stats_async(ta, tb, dc.LO)
    ev.synchronize()
    assert ops.dup_stats_decode(host) == got


# ------------------------------------------------------------------------------------------------------------------ filter
def test_filter_decisions_on_the_device(dev):
    """12 frames of 96 x 160: exact copies, copies with +-1 LSB of noise on every byte (dropped), a copy with one 8 x 8 block changed by
    40/255 (kept: one block above hi is enough), three copies in a row and a fourth (kept: --dedup-max 3)."""
    rng = np.random.default_rng(3)
    base = dc.moving_clip(6, H, W, seed=41)

    def noisy(f):
        return np.clip(f.astype(np.int16) + rng.integers(-1, 2, size=f.shape), 0, 255).astype(np.uint8)

    def patched(f):
        g = f.copy()
        blk = g[40:48, 64:72].astype(np.int16)
        g[40:48, 64:72] = np.where(blk < 128, blk + 40, blk - 40).astype(np.uint8)
        return g

    clip = [base[0], base[0].copy(), base[1], noisy(base[1]), patched(base[1]), base[2], base[3], base[3].copy(), noisy(base[3]),
            base[3].copy(), base[3].copy(), base[4]]
    src = iter(clip + [None])
    inputs = []

    def to_inp(raw):
        inputs.append(tools.to_inp(raw, (H, W)))
        return inputs[-1]

    f = driver.KeptFrames(lambda k: next(src), to_inp, dedup.Settings())
    while f.next() is not None:
        pass
    x = [t.cpu().numpy() for t in inputs]
    dups = [dc.np_is_dup(x[k - 1], x[k]) for k in range(1, 12)]
    assert dups == [True, False, True, False, False, False, True, True, True, True, False]
    assert f.kept == dedup.kept_indices(dups) == [0, 2, 4, 5, 6, 10, 11] and f.total == 12


# ------------------------------------------------------------------------------------------------------------------ command lines
PATTERN = [0, 0, 1, 2, 2, 2, 3, 4, 4, 5]  # f0 f0 f1 f2 f2 f2 f3 f4 f4 f5
PATTERN_KEPT = [0, 2, 3, 6, 7, 9]


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    """-> {job: (frames written, kept indices)} and the Y4M stream of the last job"""
    tmp = tmp_path_factory.mktemp("dedup")
    wdir = tmp / "w"
    wdir.mkdir()
    torch.save({"module." + k: v for k, v in synth.ifnet_state_dict(0).items()}, str(wdir / "flownet.pkl"))
    A = dc.moving_clip(6, H, W, seed=41)
    clips = {"A": A, "B": dc.repeat_clip(A, [i // 2 for i in range(12)]), "C": dc.repeat_clip(A, PATTERN), "D": dc.moving_clip(8, H, W, seed=42)}
    for name, fr in clips.items():
        np.savez(str(tmp / f"{name}.npz"), frames=np.stack(fr), fps=np.float64(24.0))
    jobs = [("C_dedup", "C", ["--dedup", "-fps", "60", "-s"]), ("Y", "-", ["-t", "2", "--dedup"]),
            ("A_t4", "A", ["-t", "4", "--deterministic"]), ("B_dedup", "B", ["-t", "2", "--dedup", "--deterministic"]),
            ("B_plain", "B", ["-t", "2", "--deterministic"]), ("D_dedup", "D", ["-t", "2", "--dedup", "--deterministic"]),
            ("D_plain", "D", ["-t", "2", "--deterministic"])]
    argv = [(j, ["-m", "rife", "-i", "-" if c == "-" else str(tmp / f"{c}.npz"), "-o", "-" if c == "-" else str(tmp / f"{j}.npz")] + extra)
            for j, c, extra in jobs]
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import drba_amd.infer as I\n"
        "run = I.interpolate_stream\n"
        "def reporting(*a, **k):\n"
        "    k['on_kept'] = lambda i: print('kept', i, file=sys.stderr)\n"
        "    return run(*a, **k)\n"
        "I.interpolate_stream = reporting\n"
        "m = I.load_model('rife', 1.0, weights=%r)\n"
        "for job, argv in %r:\n"
        "    print('job', job, file=sys.stderr)\n"
        "    print('written', I.inference(m, I.parse_args(argv)), file=sys.stderr)\n" % (ROOT, str(wdir), argv))
    y_in = yc.clip_from_bgr(clips["B"], 8)
    hdr = y4m.Header(W, H, (24, 1), interlace="p", chroma="420mpeg2")
    env = dict(os.environ, DRBA_TUNE_CACHE="0")
    r = subprocess.run([sys.executable, "-c", code], input=yc.y4m_bytes(y_in, hdr), capture_output=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out, job = {}, None
    for word, rest in re.findall(r"\b(job|kept|written) (\w+)", r.stderr.decode()):  # (a progress bar shares the stream and its lines)
        if word == "job":
            job = rest
            out[job] = {"kept": [], "written": None}
        elif word == "kept" and job:
            out[job]["kept"].append(int(rest))
        elif word == "written" and job:
            out[job]["written"] = int(rest)
    for j, c, _ in jobs:
        if c != "-":
            out[j]["frames"] = np.load(str(tmp / f"{j}.npz"))["frames"]
    out["Y"]["stream"] = r.stdout
    out["clips"] = clips
    return out


def _gate(got, want):
    """tests/test_gpu_cli.py's: no byte off by more than 1 LSB, fewer than 2e-3 of the bytes differ -> (ok, max, fraction)"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    return bool(d.max() <= 1 and (d > 0).mean() < 2e-3), int(d.max()), float((d > 0).mean())


def test_doubling_identity(runs):
    """B = every frame of A twice.  B at -t 2 with --dedup writes 24 frames: B[j] is A's frame j + 1 at -t 4 (all mapped timesteps
    are dyadic: 0.625, 0.875, 1.125, 1.375 in both runs) and B[23] the last source frame converted.  Without --dedup the same clip
    does not pass the gate: the motion sits in every second interval."""
    a, bd, bp = runs["A_t4"]["frames"], runs["B_dedup"]["frames"], runs["B_plain"]["frames"]
    assert runs["B_dedup"]["kept"] == [0, 2, 4, 6, 8, 10] and runs["B_dedup"]["written"] == 24 and runs["A_t4"]["written"] == 24
    assert runs["A_t4"]["kept"] == [] and runs["B_plain"]["kept"] == []  # (no filter without the flag)
    ok, mx, frac = _gate(bd[:23], a[1:])
    print(f"doubling identity: max {mx} LSB, {frac:.2e} of the bytes differ, byte-identical: {np.array_equal(bd[:23], a[1:])}")
    assert ok, (mx, frac)
    assert np.array_equal(bd[23], a[23])  # both: the last drawing, converted and written as it stands
    ok_plain, mx_p, frac_p = _gate(bp[:23], a[1:])
    print(f"without --dedup: max {mx_p} LSB, {frac_p:.2e} of the bytes differ")
    assert not ok_plain


def test_unequal_gaps_against_the_cpu_driver(runs):
    """f0 f0 f1 f2 f2 f2 f3 f4 f4 f5 with --dedup -fps 60 -s: DRBA steps over equal gaps, pairwise steps over unequal ones, fractional
    mapped timesteps -- frame for frame against the oracle driver on the CPU with the same kept indices injected."""
    import oracle
    from drba_amd import infer as drv
    from tests.clip_common import ListIO, cpu_hooks
    assert runs["C_dedup"]["kept"] == PATTERN_KEPT
    to_inp, to_out, check = cpu_hooks()
    count = iter(range(len(PATTERN)))

    def numbered(fr, size):
        x = to_inp(fr, size)
        x.k = next(count)
        return x

    io_ = ListIO(list(runs["clips"]["C"]), 24.0)
    kept = []
    drv.interpolate_stream(oracle.rife.RifeOracle(synth.ifnet_state_dict(0), 1.0), io_, 60.0, times=-1, enable_scdet=True, to_inp=numbered,
                           to_out=to_out, check_scene=check, dedup=True, check_dup=lambda a, b: b.k not in PATTERN_KEPT, on_kept=kept.append)
    assert kept == PATTERN_KEPT
    want, got = np.stack(io_.written), runs["C_dedup"]["frames"]
    assert len(want) == runs["C_dedup"]["written"] == 26  # what the plain run writes for 10 frames at 24 -> 60 fps
    ok, mx, frac = _gate(got, want)
    print(f"unequal gaps: max {mx} LSB, {frac:.2e} of the bytes differ")
    assert ok, (mx, frac)


def test_clip_without_repeats_is_unchanged(runs):
    assert runs["D_dedup"]["kept"] == list(range(8)) and runs["D_dedup"]["written"] == runs["D_plain"]["written"] == 16
    assert runs["D_dedup"]["frames"].tobytes() == runs["D_plain"]["frames"].tobytes()


def test_y4m_stream_with_dedup(runs):
    assert runs["Y"]["kept"] == [0, 2, 4, 6, 8, 10] and runs["Y"]["written"] == 24
    rd = y4m.Reader(io.BytesIO(runs["Y"]["stream"]))
    frames = list(rd)
    assert (rd.header.width, rd.header.height, rd.header.fps_num, rd.header.fps_den) == (W, H, 48, 1)
    assert len(frames) == 24 and all(f.depth == 8 for f in frames)
