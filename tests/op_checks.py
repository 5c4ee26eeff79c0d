"""Per-operator fp64 parity checks of the GMFlow / GMFSS glue kernels (gmflow.hip, gmfss_glue.hip, the small kernels of
splat_warp.hip and the layout kernels of ifnet_glue.hip and frame_io.hip), of the generic forward splat (splat_warp.hip:
drba_softsplat, _index, _again, _gather_quad), of resize_bilinear_scale and flow_distance, and of the IFNet stage glue
(ifnet_glue.hip, flow_terms.hpp, stage_conv.hip, stage_conv16.hip: stage-input gathers, the gathers fused with conv0[0], the
flow update, the final warp + blend -- in the forms the pipeline runs them), and of the 3x3 convolution's epilogue forms with
every configuration id pinned (conv.hip, conv_split.hip, conv_dma.hip, conv_ks.hip; CONV_FORMS below), and of the three
GMFlow transformer kernels at their dispatch edges (window_attn.hip, global_corr.hip, linear_split.hip; ATTN_CASES, GCORR_MAPS,
LIN_EDGES below), and of IFNet's context encoder as one kernel in its two forms at every tile, border and store edge (head_fused.hip,
head_fused16.hip; HEAD_CASES below), and of the fused RIFE splats -- the pre-pass / tile kernel pair behind flow_reverse and the
linear and non-linear DRM maps -- at every halo, window and spill edge (splat_warp.hip; rife_cases below), shared by
tests/test_gpu_op_parity.py, tests/test_op_checks_cpu.py and the diagnostic report (python -m tests.gpu_report).

Every check takes the device the inputs go to and the `ops` namespace under test (default: drba_amd.ops; the CPU test hands
in a torch stand-in, with and without a planted defect) and returns rows (name, err, tol, extra) with the pass rule of every
parity row, `err <= tol`.

References are plain torch on the CPU in float64, written from the formulas of the reference model that the kernel comments
cite (oracle/*.py restates them), never from the kernels.  Value rows use one rule,

    tol = max(2e-5 * max(1, |ref|max), 3 * floor),

where `floor` is the max error of the fp32 oracle / fp32 torch evaluation of the same formula on the same input against the
fp64 reference: measured per row, printed in the row, never calibrated against the code under test.  Decisions (masks, hole
tests, the DRM retiming walk) and pure data movement are compared bit for bit: err = number of differing elements, tol = 0.  The transformer rows keep three bars of their own, named in
Row.tol_rule: a two-term attention row max(rule, 3 x the format floor: the fp64 formula on operands rounded to two fp16 terms), the
coordinate rows of global_expect2 and the linear_split rows the bars tests/gpu_checks.py already holds those kernels to.  The fused
encoder's two-term rows stay on the one rule: their format floor is printed, and the CPU suite asserts that three times it is below the rule.

Three places where ATen's CPU result is not the specification are written out instead of taken from ATen:
  * a zeros-padding bilinear sample at a non-finite coordinate is 0 (every tap is outside the image; ATen's CPU kernel forms
    0 * NaN there, its CUDA kernel -- what the reference model runs on -- skips the taps);
  * InstanceNorm of a one-element plane is 0 (variance 0; F.instance_norm refuses the shape);
  * a bilinear resize by 1 (the scale-1 stage's interpolate(x, scale_factor=1)) is the identity, also at a non-finite pixel
    (_down; ATen's weight-0 tap makes a NaN of it, at the pixel on the CPU and at its neighbour on the GPU).
A stage input is reported as one row per channel group (frames, features, timestep, mask / feat, flow: magnitudes 1, 4, 1, 3
and up to thousands), each with its own |ref|max and floor, so that the flow channels do not set what the frames are allowed.
The splat's reference takes its targets as the specification does, as the fp32 sum x + flow, and evaluates everything after
that in fp64 (softsplat_ref): with fp64 targets a source next to an integer lands on other pixels than the specified ones, and
the fp32 oracle's "error" against such a reference (1e-4 at 37 x 83, above 1 for avg at 1024 x 1280) would set a tolerance
that detects nothing.  A finite target beyond the int32 range contributes nothing (softsplat_ref), and flow_distance is +inf
where the fp32 squares overflow (flow_distance_ref).
Inputs regenerate from seeds (cases.rnd, synth._smooth_field)."""
import collections
import math

import torch
import torch.nn.functional as F

from drba_amd.utils import synth
from oracle import drm as odrm
from oracle import gmflow as ogm
from oracle import ops as oops
from tests import cases


class Row(tuple):
    """(name, err, tol, extra) -- what _assert_rows / report.record / gpu_report take -- that also carries the operator family,
    the measured fp32 floor and |ref|max of a value row (None for bit-exact rows)."""

    def __new__(cls, op, name, err, tol, extra="", floor=None, refmax=None):
        self = super().__new__(cls, (f"{op} {name}", err, tol, extra))
        self.op, self.floor, self.refmax = op, floor, refmax
        return self


def default_ops():
    from drba_amd import ops
    return ops


def rule_tol(refmax, floor):
    return max(2e-5 * max(1.0, refmax), 3.0 * floor)


def _err(got, ref):
    """max |got - ref| in float64 over the elements where ref is finite; inf when the shapes differ or the non-finite elements
    of ref (NaN, +inf, -inf) are not the same values at the same places in got."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    if g.shape != r.shape:
        return float("inf")
    fin = torch.isfinite(r)
    if not torch.equal(torch.isfinite(g), fin):
        return float("inf")
    if not bool(fin.all()):
        gn, rn = g[~fin], r[~fin]
        if not (torch.equal(gn.isnan(), rn.isnan()) and torch.equal(torch.nan_to_num(gn, 0.0, 1.0, -1.0), torch.nan_to_num(rn, 0.0, 1.0, -1.0))):
            return float("inf")
    d = (g[fin] - r[fin]).abs()
    return float(d.max()) if d.numel() else 0.0


def value_row(op, name, got, ref64, ref32, extra=""):
    fin = ref64[torch.isfinite(ref64)]
    refmax = float(fin.abs().max()) if fin.numel() else 0.0
    floor = _err(ref32, ref64)
    return Row(op, name, _err(got, ref64), rule_tol(refmax, floor), f"fp32_floor={floor:.2e} |ref|max={refmax:.3g} {extra}".rstrip(),
               floor, refmax)


def _mismatches(got, want):
    """elements that differ bit for bit (any NaN equals any NaN; -0 differs from +0)"""
    g, w = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    if g.shape != w.shape or g.dtype != w.dtype:
        return float("inf")
    if g.dtype == torch.float32:
        same = (g.view(torch.int32) == w.view(torch.int32)) | (g.isnan() & w.isnan())
    else:
        same = g == w
    return float((~same).sum())


def exact_row(op, name, got, want, extra=""):
    return Row(op, name, _mismatches(got, want), 0.0, f"bit-exact, {want.numel()} elements {extra}".rstrip())


def _smooth(c, h, w, seed):
    return synth._smooth_field(c, h, w, seed)


# ----------------------------------------------------------------------------------------- softmax_rows_
SOFTMAX_COLS = (1, 2, 63, 64, 65, 576, 577, 1024, 1025, 2304, 2305, 8704, 8705)  # both sides of every dispatch bound of drba_softmax_rows
SOFTMAX_MASKED = (35, 700, 2000, 5000, 9000)  # one per dispatch branch (<= 576, <= 1024, <= 2304, <= 8704, the three-pass kernel)


def block_mask(n_masks, rows, cols, seed):
    """[n_masks, rows, cols] of 0 / -100 the way shift_window_mask builds it: -100 where the row's and the column's region
    labels differ (transformer.py:19-43), with seeded labels so that rows != cols is possible."""
    g = torch.Generator().manual_seed(seed)
    rl = torch.randint(0, 3, (n_masks, rows, 1), generator=g)
    cl = torch.randint(0, 3, (n_masks, 1, cols), generator=g)
    cl[:, :, 0] = rl[:, 0]  # (no row of the first label is masked everywhere)
    m = torch.zeros(n_masks, rows, cols)
    return m.masked_fill(rl != cl, -100.0)


def _softmax_ref(scores, scale, mask):
    s = scores / scale
    if mask is not None:
        m, n = scores.shape[0], mask.shape[0]
        s = s + mask.to(s.dtype).repeat((m + n - 1) // n, 1, 1)[:m]  # matrix i takes mask i % n_masks (transformer.py:85)
    return torch.softmax(s, dim=-1)


def check_softmax_rows(dev, ops=None):
    ops = ops or default_ops()
    op, rows = "softmax_rows_", []

    def one(name, scores, scale, mask):
        got = ops.softmax_rows_(scores.to(dev).clone(), scale, None if mask is None else mask.to(dev))
        rows.append(value_row(op, name, got, _softmax_ref(scores.double(), scale, mask), _softmax_ref(scores, scale, mask)))

    for k, cols in enumerate(SOFTMAX_COLS):  # 3 matrices of 5 rows: 15 rows, the last block of 4 is partial
        one(f"cols={cols} [3x5 rows]", cases.rnd((3, 5, cols), 300 + k, 3.0), 1.0, None)
    for k, cols in enumerate(SOFTMAX_MASKED):  # 5 matrices cycle 2 masks (5 % 2 != 0), 3 rows each
        one(f"cols={cols} masked [5x3 rows, 2 masks]", cases.rnd((5, 3, cols), 320 + k, 3.0), 1.0, block_mask(2, 3, cols, 330 + k))
    # the mask of a real shifted 2 x 2 split of a 10 x 14 map (5 x 7 windows: L = cols = 35), 7 matrices over its 4 masks
    one("cols=35 shift_window_mask [7x35 rows, 4 masks]", cases.rnd((7, 35, 35), 340, 3.0), 1.0, ogm.shift_window_mask(10, 14, 5, 7, 2, 3))
    one("cols=65 |scores|~80", cases.rnd((3, 5, 65), 341, 80.0), 1.0, None)
    one("cols=700 scale=sqrt(128)", cases.rnd((3, 5, 700), 342, 30.0), 128 ** 0.5, block_mask(2, 5, 700, 343))
    return rows


# ----------------------------------------------------------------------------------------- instance_norm
IN_PLANES = ((1, 1), (1, 5), (1, 31), (4, 8), (3, 11), (37, 53), (144, 240))  # HW = 1, 5, 31, 32, 33, 37*53, 144*240


def _inorm_ref(x, relu):
    if x.shape[2] * x.shape[3] == 1:
        y = torch.zeros_like(x)  # one element: it is its own mean
    else:
        y = F.instance_norm(x, eps=1e-5)  # backbone.py:7,17-20
    return F.relu(y) if relu else y


def check_instance_norm(dev, ops=None):
    ops = ops or default_ops()
    op, rows = "instance_norm", []

    def one(name, x, relu):
        got = ops.instance_norm(x.to(dev), relu=relu)
        rows.append(value_row(op, f"{name} relu={int(relu)}", got, _inorm_ref(x.double(), relu), _inorm_ref(x, relu)))

    for k, (h, w) in enumerate(IN_PLANES):
        one(f"1x1x{h}x{w}", cases.rnd((1, 1, h, w), 400 + k, 2.0) + 0.3, relu=bool(k % 2))
        one(f"2x3x{h}x{w}", cases.rnd((2, 3, h, w), 420 + k, 2.0) + 0.3, relu=not k % 2)
    one("2x3x37x53", cases.rnd((2, 3, 37, 53), 440, 2.0), relu=True)
    one("1x1x37x53", cases.rnd((1, 1, 37, 53), 441, 2.0), relu=True)
    # a mean that dwarfs the spread: the fp32 inputs (exact in the fp64 reference) sit ~160 ulps apart at most
    one("2x3x37x53 mean 1e3 std 1e-2", cases.rnd((2, 3, 37, 53), 442, 1e-2) + 1e3, relu=False)
    one("1x2x144x240 mean 1e3 std 1e-2", cases.rnd((1, 2, 144, 240), 443, 1e-2) + 1e3, relu=False)
    x = cases.rnd((1, 3, 37, 53), 444, 1.0)
    x[0, 1] = 3.7  # a constant plane: variance 0, the output is 0 (and finite)
    one("1x3x37x53 constant plane", x, relu=False)
    got = ops.instance_norm(x.to(dev), relu=False)[0, 1]
    rows.append(value_row(op, "constant plane alone -> 0", got, torch.zeros(37, 53, dtype=torch.float64), F.instance_norm(x, eps=1e-5)[0, 1]))
    return rows


# ----------------------------------------------------------------------------------------- conv_direct
CONV_CASES = (  # (n, cin, cout, h, w, k, stride, pad, bias)
    (1, 3, 64, 37, 61, 7, 2, 3, False), (1, 3, 64, 128, 256, 7, 2, 3, False), (2, 7, 70, 11, 19, 7, 2, 3, True),
    (3, 5, 17, 13, 45, 3, 1, 1, True), (3, 5, 15, 13, 45, 3, 2, 1, True), (1, 6, 1, 9, 13, 3, 1, 1, False),
    (1, 3, 70, 37, 61, 1, 1, 0, True), (3, 6, 17, 9, 13, 1, 1, 0, True), (3, 6, 15, 9, 13, 1, 2, 0, False),  # Cin % 4 != 0: not the MFMA path
    (3, 8, 70, 9, 13, 1, 1, 0, True), (1, 8, 15, 5, 7, 1, 2, 0, False), (3, 8, 1, 9, 13, 1, 1, 0, True), (1, 8, 17, 37, 61, 1, 1, 0, True))


def check_conv_direct(dev, ops=None):
    ops = ops or default_ops()
    rows = []
    for i, (n, cin, cout, h, w, k, s, p, has_b) in enumerate(CONV_CASES):
        x = cases.rnd((n, cin, h, w), 500 + i, 1.0)
        wt = cases.rnd((cout, cin, k, k), 530 + i, 1.0 / (cin * k * k) ** 0.5)
        b = cases.rnd((cout,), 560 + i, 0.5) if has_b else None
        got = ops.conv_direct(x.to(dev), wt.to(dev), None if b is None else b.to(dev), s, p)
        ref64 = F.conv2d(x.double(), wt.double(), None if b is None else b.double(), stride=s, padding=p)
        rows.append(value_row("conv_direct", f"[{n}x{cin}->{cout} {h}x{w} k{k} s{s} p{p} bias={int(has_b)}]", got, ref64,
                              F.conv2d(x, wt, b, stride=s, padding=p)))
    return rows


# ----------------------------------------------------------------------------------------- local_corr_flow
LCORR_CASES = ((128, 1, 1), (128, 3, 70), (128, 13, 45), (128, 33, 64), (128, 65, 31),  # the MFMA kernel: width below / at / past a 64 tile
               (96, 1, 1), (96, 3, 70), (96, 13, 45), (96, 33, 64), (96, 65, 31),        # the generic kernel (32-pixel tiles)
               (32, 1, 1), (32, 13, 45), (32, 33, 64), (130, 3, 70), (130, 65, 31))


def _lcorr_ref(f0, f1, r):
    if f0.shape[2] == 1 and f0.shape[3] == 1:
        return torch.zeros(1, 2, 1, 1, dtype=f0.dtype)  # one pixel: only the centre tap is in the image (matching.py:41-89 divides by W - 1)
    return ogm.local_correlation_softmax(f0, f1, r)


def check_local_corr_flow(dev, ops=None):
    ops = ops or default_ops()
    op, rows = "local_corr_flow", []

    def one(name, f0, f1):
        got = ops.local_corr_flow(f0.to(dev), f1.to(dev), 4)
        rows.append(value_row(op, name, got, _lcorr_ref(f0.double(), f1.double(), 4), _lcorr_ref(f0, f1, 4)))

    for i, (c, h, w) in enumerate(LCORR_CASES):
        one(f"C={c} {h}x{w}", cases.rnd((1, c, h, w), 600 + i, 0.6), cases.rnd((1, c, h, w), 630 + i, 0.6))
    for i, (c, h, w) in enumerate(((128, 13, 45), (96, 33, 64))):
        # feature1 is feature0 moved by (+2, -1): that tap scores |f|^2 / sqrt(C) ~ 2.25 sqrt(C), the rest ~ N(0, 2.25^2)
        f0 = cases.rnd((1, c, h, w), 660 + i, 1.5)
        one(f"C={c} {h}x{w} one tap dominates", f0, torch.roll(f0, shifts=(2, -1), dims=(2, 3)).contiguous())
    return rows


# ----------------------------------------------------------------------------------------- local_attn_flow
LATTN_CASES = ((128, 1, 36, 60), (128, 4, 13, 45), (128, 4, 5, 7), (96, 1, 13, 45), (96, 4, 36, 60), (70, 4, 13, 45), (70, 1, 5, 7))


def local_attn_ref(q_tok, k_tok, flow, r):
    """transformer.py:374-409 in the F.unfold form of oracle/gmflow.py:219-225: keys and flow zero-padded, every one of the
    (2r+1)^2 window positions takes part in the softmax (an out-of-image key scores 0, it is not masked)."""
    _, _, h, w = flow.shape
    c = q_tok.shape[-1]
    q = q_tok.reshape(h * w, 1, c)
    ks = 2 * r + 1
    kp = k_tok.reshape(1, h * w, c).permute(0, 2, 1).reshape(1, c, h, w)
    kw = F.unfold(kp, kernel_size=ks, padding=r).view(1, c, ks ** 2, h, w).permute(0, 3, 4, 1, 2).reshape(h * w, c, ks ** 2)
    fw = F.unfold(flow, kernel_size=ks, padding=r).view(1, 2, ks ** 2, h, w).permute(0, 3, 4, 2, 1).reshape(h * w, ks ** 2, 2)
    prob = torch.softmax(torch.matmul(q, kw) / (c ** 0.5), dim=-1)
    return torch.matmul(prob, fw).view(1, h, w, 2).permute(0, 3, 1, 2).contiguous()


def check_local_attn_flow(dev, ops=None):
    ops = ops or default_ops()
    rows = []
    for i, (c, r, h, w) in enumerate(LATTN_CASES):
        q, k = cases.rnd((h * w, c), 700 + i, 1.2), cases.rnd((h * w, c), 720 + i, 1.2)
        flow = cases.rnd((1, 2, h, w), 740 + i, 10.0)
        got = ops.local_attn_flow(q.to(dev), k.to(dev), flow.to(dev), r)
        rows.append(value_row("local_attn_flow", f"C={c} r={r} {h}x{w}", got, local_attn_ref(q.double(), k.double(), flow.double(), r),
                              local_attn_ref(q, k, flow, r)))
    return rows


# ----------------------------------------------------------------------------------------- convex_upsample
CONVEX_CASES = ((4, 1, 1), (4, 5, 7), (4, 36, 60), (2, 5, 7), (2, 36, 60), (8, 1, 1), (8, 5, 7), (8, 13, 45))


def convex_upsample_ref(mask, flow, factor):
    """gmflow.py:76-89 (oracle/gmflow.py:232-236): softmax over the 9 taps of mask [1, 9 K K, h, w], weighted sum of the 3 x 3
    zero-padded neighbourhood of K * flow, sub-pixel (ii, jj) of mask channel (t K + ii) K + jj goes to (K y + ii, K x + jj)."""
    b, fc, h, w = flow.shape
    m = torch.softmax(mask.view(b, 1, 9, factor, factor, h, w), dim=2)
    up = F.unfold(factor * flow, [3, 3], padding=1).view(b, fc, 9, 1, 1, h, w)
    up = torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3)
    return up.reshape(b, fc, factor * h, factor * w)


def check_convex_upsample(dev, ops=None):
    ops = ops or default_ops()
    rows = []
    for i, (k, h, w) in enumerate(CONVEX_CASES):
        mask, flow = cases.rnd((1, 9 * k * k, h, w), 800 + i, 5.0), cases.rnd((1, 2, h, w), 820 + i, 3.0)
        got = ops.convex_upsample(mask.to(dev), flow.to(dev), k)
        rows.append(value_row("convex_upsample", f"x{k} {h}x{w}", got, convex_upsample_ref(mask.double(), flow.double(), k),
                              convex_upsample_ref(mask, flow, k)))
    return rows


# ----------------------------------------------------------------------------------------- flow_warp / backwarp
WARP_MAPS = ((2, 2), (13, 45), (37, 83))


def _nonfinite_to_zero(out, flow):
    bad = ~(torch.isfinite(flow[:, 0:1]) & torch.isfinite(flow[:, 1:2]))
    return torch.where(bad, torch.zeros_like(out), out)


def flow_warp_ref(x, flow):
    return _nonfinite_to_zero(ogm.flow_warp(x, flow), flow)  # geometry.py:53-84


def backwarp_ref(x, flow, padding):
    """warplayer.py:8-22 (border) / MetricNet.py:10-20 (zeros) as oracle/ops.py states them, the base grid made in the dtype
    of the inputs (the oracle's is always fp32)."""
    n, _, h, w = flow.shape
    gx = torch.linspace(-1.0, 1.0, w, dtype=x.dtype).view(1, 1, 1, w).expand(n, 1, h, w)
    gy = torch.linspace(-1.0, 1.0, h, dtype=x.dtype).view(1, 1, h, 1).expand(n, 1, h, w)
    fx = flow[:, 0:1] / ((w - 1.0) / 2.0)
    fy = flow[:, 1:2] / ((h - 1.0) / 2.0)
    grid = (torch.cat([gx, gy], 1) + torch.cat([fx, fy], 1)).permute(0, 2, 3, 1)
    out = F.grid_sample(x, grid, mode="bilinear", padding_mode=padding, align_corners=True)
    return _nonfinite_to_zero(out, flow) if padding == "zeros" else out


def warp_flows(n, h, w, seed):
    """name -> flow [n, 2, h, w]: smooth, mostly out of the image, and exactly integer (with the last row / column, one past
    them, far outside, and an infinite component)."""
    flows = {"smooth": (_smooth(2 * n, h, w, seed).view(n, 2, h, w) - 0.5) * 8.0, "amp30": cases.rnd((n, 2, h, w), seed + 1, 30.0)}
    g = torch.Generator().manual_seed(seed + 2)
    f = torch.randint(-3, 4, (n, 2, h, w), generator=g).float()
    f[:, 0, 0, 0], f[:, 1, 0, 0] = w - 1.0, h - 1.0       # (0, 0) samples the last column of the last row
    f[:, 0, 0, 1], f[:, 1, 0, 1] = w - 1.0, 0.0           # (1, 0): one past the last column
    f[:, 0, 1, 0], f[:, 1, 1, 0] = 0.0, h - 1.0           # (0, 1): one past the last row
    f[:, 0, 1, 1], f[:, 1, 1, 1] = -2.0, -2.0             # (1, 1): one before the first row and column
    if h > 2:
        f[:, 0, 2, 3], f[:, 1, 2, 3] = float("inf"), 1.0
        f[:, 0, 3, 2], f[:, 1, 3, 2] = 1.0, float("-inf")
        f[:, 0, 4, 4], f[:, 1, 4, 4] = -1000.0, 2000.0
    else:
        f[:, 0, 1, 1] = float("inf")
    flows["integer"] = f
    return flows


def check_flow_warp(dev, ops=None):
    ops = ops or default_ops()
    rows = []
    for i, (c, (h, w)) in enumerate(((1, WARP_MAPS[0]), (16, WARP_MAPS[0]), (16, WARP_MAPS[1]), (128, WARP_MAPS[1]), (1, WARP_MAPS[2]),
                                     (16, WARP_MAPS[2]), (128, WARP_MAPS[2]))):
        x = cases.rnd((1, c, h, w), 900 + i, 1.0)
        for name, flow in warp_flows(1, h, w, 920 + 3 * i).items():
            got = ops.flow_warp(x.to(dev), flow.to(dev))
            rows.append(value_row("flow_warp", f"C={c} {h}x{w} {name}", got, flow_warp_ref(x.double(), flow.double()), flow_warp_ref(x, flow)))
    return rows


def check_backwarp(dev, ops=None):
    ops = ops or default_ops()
    rows = []
    for i, (n, c, (h, w)) in enumerate(((1, 1, WARP_MAPS[0]), (2, 16, WARP_MAPS[0]), (1, 16, WARP_MAPS[1]), (2, 128, WARP_MAPS[1]),
                                        (2, 1, WARP_MAPS[2]), (1, 128, WARP_MAPS[2]))):
        x = cases.rnd((n, c, h, w), 1000 + i, 1.0)
        for name, flow in warp_flows(n, h, w, 1020 + 3 * i).items():
            for padding in ("zeros", "border"):
                got = ops.backwarp(x.to(dev), flow.to(dev), padding)
                rows.append(value_row("backwarp", f"{padding} N={n} C={c} {h}x{w} {name}", got, backwarp_ref(x.double(), flow.double(), padding),
                                      backwarp_ref(x, flow, padding)))
    return rows


# ----------------------------------------------------------------------------------------- resize_bilinear_ac
RESIZE_CASES = (  # (nc, hin, win, hout, wout, mul)
    (6, 18, 30, 36, 60, 2.0), (6, 36, 60, 18, 30, 1.0), (6, 13, 45, 13, 45, 2.0), (6, 13, 45, 1, 45, 1.0), (6, 13, 45, 13, 1, 2.0),
    (6, 13, 45, 1, 1, 2.0), (6, 1, 45, 7, 90, 2.0), (6, 1, 1, 5, 7, 1.0), (2, 72, 120, 144, 240, 2.0), (6, 37, 53, 50, 31, 1.0))


def resize_ac_ref(x, size, mul):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=True) * mul  # gmflow.py:131


def check_resize_bilinear_ac(dev, ops=None):
    ops = ops or default_ops()
    rows = []
    for i, (nc, hi, wi, ho, wo, mul) in enumerate(RESIZE_CASES):
        shape = (nc // 2, 2, hi, wi) if nc % 2 == 0 and i % 2 else (1, nc, hi, wi)
        x = cases.rnd(shape, 1100 + i, 2.0)
        got = ops.resize_bilinear_ac(x.to(dev), (ho, wo), mul)
        rows.append(value_row("resize_bilinear_ac", f"NC={nc} {hi}x{wi}->{ho}x{wo} mul={mul:g}", got, resize_ac_ref(x.double(), (ho, wo), mul),
                              resize_ac_ref(x, (ho, wo), mul)))
    return rows


# ----------------------------------------------------------------------------------------- layernorm / gelu / bmm / pointwise
BIG = (1 << 20) + 77  # above kMaxBlocks * 256 elements: the grid-stride loops go round more than once
SMALL = 1000          # not a multiple of the 256-thread block
BIG_MAP = (1025, 1031)  # the same for the kernels whose loop runs over the pixels of one sample


def check_layernorm(dev, ops=None):
    ops = ops or default_ops()
    rows = []
    for i, (nrows, cols) in enumerate(((5, 1), (7, 63), (5, 64), (6, 65), (13, 128), (3, 200), (1, 128))):
        x = cases.rnd((nrows, cols), 1200 + i, 2.0) + 0.5
        w, b = cases.rnd((cols,), 1220 + i, 1.0), cases.rnd((cols,), 1240 + i, 0.5)
        for res in (None, cases.rnd((nrows, cols), 1260 + i, 1.0)):
            got = ops.layernorm(x.to(dev), w.to(dev), b.to(dev), residual=None if res is None else res.to(dev))
            ref64 = F.layer_norm(x.double(), (cols,), w.double(), b.double())
            ref32 = F.layer_norm(x, (cols,), w, b)
            if res is not None:
                ref64, ref32 = res.double() + ref64, res + ref32
            rows.append(value_row("layernorm", f"{nrows}x{cols} residual={int(res is not None)}", got, ref64, ref32))
    return rows


def check_gelu(dev, ops=None):
    ops = ops or default_ops()
    inf = float("inf")
    x = torch.cat([torch.linspace(-6.0, 6.0, 4801), torch.tensor([0.0, -0.0, 6.0, -6.0, inf, -inf, 1e-30, -1e-30, 30.0, -30.0]),
                   cases.rnd((2000,), 1300, 2.0).clamp(-6, 6)])
    # (the fp32 floor is the erf formula of nn.GELU written out: ATen's vectorised fp32 CPU gelu answers NaN at +inf, where the
    # formula and ATen's own fp64 give +inf; at -inf both give -inf * 0 = NaN)
    g32 = lambda v: 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))  # noqa: E731
    rows = [value_row("gelu", f"|x|<=6, 0, +-inf [{x.numel()}]", ops.gelu(x.to(dev)), F.gelu(x.double()), g32(x))]
    xb = cases.rnd((BIG,), 1301, 2.0)
    rows.append(value_row("gelu", f"[{BIG}]", ops.gelu(xb.to(dev)), F.gelu(xb.double()), g32(xb)))
    return rows


def check_bmm(dev, ops=None):
    ops = ops or default_ops()
    rows = []
    for i, (bs, m, n, k) in enumerate(((1, 1, 1, 1), (3, 7, 5, 130), (2, 130, 3, 17), (5, 33, 129, 65), (2, 1, 130, 1), (1, 65, 1, 127))):
        for trans_b in (True, False):
            a = cases.rnd((bs, m, k), 1400 + i, 1.0)
            b = cases.rnd((bs, n, k) if trans_b else (bs, k, n), 1420 + i, 1.0)
            got = ops.bmm(a.to(dev), b.to(dev), trans_b)
            mm = lambda p, q: torch.matmul(p, q.transpose(1, 2) if trans_b else q)  # noqa: E731
            rows.append(value_row("bmm", f"[{bs}x{m}x{k}] x [{n if trans_b else k}x{k if trans_b else n}] trans_b={int(trans_b)}", got,
                                  mm(a.double(), b.double()), mm(a, b)))
    return rows


def check_pointwise(dev, ops=None):
    """add_act, channel_normalize3, mul_map, affine (values) and clamp (bit-exact)."""
    ops = ops or default_ops()
    rows = []
    for n in (SMALL, BIG):
        a, b = cases.rnd((n,), 1500, 2.0), cases.rnd((n,), 1501, 2.0)
        for relu in (False, True):
            ref = lambda p, q: F.relu(p + q) if relu else p + q  # noqa: E731  (backbone.py:36 / gmflow.py flow + pred)
            rows.append(value_row("add_act", f"[{n}] relu={int(relu)}", ops.add_act(a.to(dev), b.to(dev), relu=relu), ref(a.double(), b.double()), ref(a, b)))
        for mul, add in ((2.0, 0.0), (-0.37, 1.0)):
            rows.append(value_row("affine", f"[{n}] *{mul:g} +{add:g}", ops.affine(a.to(dev), mul, add), a.double() * mul + add, a * mul + add))
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    m32, s32 = torch.tensor(mean).view(1, 3, 1, 1), torch.tensor(std).view(1, 3, 1, 1)  # gmflow.py:13-18: fp32 tensors
    for shape in ((1, 3, 9, 37), (2, 3, 419, 419)):
        x = torch.rand(shape, generator=torch.Generator().manual_seed(1510))
        rows.append(value_row("channel_normalize3", f"{list(shape)}", ops.channel_normalize3(x.to(dev), mean, std), (x.double() - m32.double()) / s32.double(),
                              (x - m32) / s32))
    for shape in ((2, 5, 13, 45), (1, 2) + BIG_MAP):
        x, m = cases.rnd(shape, 1520, 1.0), cases.rnd((shape[0], 1) + shape[2:], 1521, 1.0)
        rows.append(value_row("mul_map", f"{list(shape)}", ops.mul_map(x.to(dev), m.to(dev)), x.double() * m.double(), x * m))
    inf, nan, lo, hi = float("inf"), float("nan"), -0.5, 0.75
    edge = torch.tensor([nan, inf, -inf, lo, hi, -0.0, 0.0, 0.75000006, 0.74999994, -0.50000006, -0.49999997, 1e38, -1e38, 1e-45])
    for n in (SMALL, BIG):
        x = torch.cat([edge, cases.rnd((n - edge.numel(),), 1530, 1.0)])
        rows.append(exact_row("clamp", f"[{n}] NaN, +-inf, the bounds", ops.clamp(x.to(dev), lo, hi), torch.clamp(x, lo, hi)))
    return rows


# ----------------------------------------------------------------------------------------- layout kernels
def check_layouts(dev, ops=None):
    """pixel_shuffle2, pair_interleaved, quad_interleaved, rgbx and the [H, W, 4] copy ops.to_inp attaches: pure data movement,
    bit-exact against torch indexing."""
    ops = ops or default_ops()
    rows = []
    for i, shape in enumerate(((2, 12, 5, 7), (1, 4, 37, 53), (3, 8, 1, 1), (1, 16, 13, 45))):
        x = cases.rnd(shape, 1600 + i, 1.0)
        rows.append(exact_row("pixel_shuffle2", f"{list(shape)}", ops.pixel_shuffle2(x.to(dev)), F.pixel_shuffle(x, 2)))
    for i, (c, h, w) in enumerate(((16, 13, 45), (2, 1, 1), (6, 37, 53))):
        x = cases.rnd((1, c, h, w), 1610 + i, 1.0)
        want = x[0].view(c // 2, 2, h, w).permute(0, 2, 3, 1).contiguous()
        rows.append(exact_row("pair_interleaved", f"[1, {c}, {h}, {w}]", ops.pair_interleaved(x.to(dev)), want))
    for i, (n, c, h, w) in enumerate(((1, 16, 13, 45), (2, 20, 37, 53), (3, 16, 1, 1))):
        x = cases.rnd((n, c, h, w), 1620 + i, 1.0)
        want = x.view(n, c // 4, 4, h * w).permute(0, 1, 3, 2).contiguous()
        rows.append(exact_row("quad_interleaved", f"[{n}, {c}, {h}, {w}]", ops.quad_interleaved(x.to(dev)), want))
    for i, (h, w) in enumerate(((13, 45), (1, 1), (37, 53))):
        x = cases.rnd((1, 3, h, w), 1630 + i, 1.0)
        want = torch.cat([x[0].permute(1, 2, 0), torch.zeros(h, w, 1)], 2).contiguous()
        rows.append(exact_row("rgbx", f"[1, 3, {h}, {w}]", ops.rgbx(x.to(dev)), want))
    for i, ((h, w), (ho, wo)) in enumerate((((37, 53), (37, 53)), ((37, 53), (64, 96)), ((45, 83), (32, 64)))):
        img = torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(1640 + i), dtype=torch.uint8)
        out = ops.to_inp(img.to(dev), (ho, wo))
        x4 = getattr(out, "_drba_x4", None)
        if x4 is None or x4[1] != out._version:
            rows.append(Row("to_inp", f"x4 copy {h}x{w}->{ho}x{wo}", float("inf"), 0.0, "no current _drba_x4 copy on the frame"))
            continue
        want = torch.cat([out[0].detach().cpu().permute(1, 2, 0), torch.zeros(ho, wo, 1)], 2).contiguous()
        rows.append(exact_row("to_inp", f"x4 copy {h}x{w}->{ho}x{wo}", x4[0], want))
    return rows


# ----------------------------------------------------------------------------------------- hole tests
def cover_values(n, seed):
    """Cover maps around the 0.999f hole test: exactly 0.999f, its two fp32 neighbours, 0, 1, NaN, +-inf, then seeded values."""
    t = torch.tensor(0.999, dtype=torch.float32)
    one = torch.tensor(1.0)
    edge = torch.stack([t, torch.nextafter(t, one), torch.nextafter(t, -one), torch.tensor(0.0), one, torch.tensor(float("nan")),
                        torch.tensor(float("inf")), torch.tensor(float("-inf")), torch.tensor(0.9989), torch.tensor(0.9991)])
    g = torch.Generator().manual_seed(seed)
    return torch.cat([edge, 0.99 + 0.012 * torch.rand(n - edge.numel(), generator=g)])


def check_hole_tests(dev, ops=None):
    """timestep_fix (GMFSS.py:120-122) and fill_holes (drm.py: torch.where(cover < 0.999, value, aligned)): bit-exact."""
    ops = ops or default_ops()
    rows = []
    for n in (SMALL, BIG):
        c0 = cover_values(n, 1700).view(1, 1, 1, n)
        c1 = torch.roll(cover_values(n, 1701), 16).view(1, 1, 1, n)  # the edge values of one map meet ordinary values of the other
        t0, t1 = cases.rnd((1, 1, 1, n), 1702, 1.0), cases.rnd((1, 1, 1, n), 1703, 1.0)
        o0, o1 = ops.timestep_fix(t0.to(dev), t1.to(dev), c0.to(dev), c1.to(dev))
        bad = (c0 < 0.999) | (c1 < 0.999)
        rows.append(exact_row("timestep_fix", f"[{n}] out0", o0, torch.where(bad, torch.ones_like(t0), t0)))
        rows.append(exact_row("timestep_fix", f"[{n}] out1", o1, torch.where(bad, torch.ones_like(t1), t1)))
        assert 0 < int(bad.sum()) < n
        got = ops.fill_holes(t0.to(dev), c0.to(dev), t1.to(dev))
        rows.append(exact_row("fill_holes", f"[{n}]", got, torch.where(c0 < 0.999, t1, t0)))
    return rows


# ----------------------------------------------------------------------------------------- drm
def check_drm(dev, ops=None):
    """drm_ratio against oracle.drm's ratio maps (the distances in fp32, as the reference computes them: tools.py:77-80) and
    drm_retime bit for bit against the fp32 walk of oracle.drm.drm_to_t (a chain of roundings, no tolerance against fp64)."""
    ops = ops or default_ops()
    rows = []
    for i, (n, h, w) in enumerate(((1, 37, 53), (2, 37, 53), (1,) + BIG_MAP)):
        f10, f12 = cases.rnd((n, 2, h, w), 1800 + i, 5.0), cases.rnd((n, 2, h, w), 1810 + i, 3.0)
        f10[:, :, 3, 4] = 0.0
        f12[:, :, 3, 4] = 0.0  # both flows zero: 0 / 0 = NaN without eps (drm.py:110-155), 0.5 with it
        f10[:, :, 5, 6] = 0.0   # one of them zero: ratio 0 / 1
        for eps in (1e-4, 0.0):
            r10, r12 = ops.drm_ratio(f10.to(dev), f12.to(dev), eps)
            w10, w12 = odrm._ratio_maps(f10.double(), f12.double(), eps)
            v10, v12 = odrm._ratio_maps(f10, f12, eps)
            rows.append(value_row("drm_ratio", f"{n}x{h}x{w} eps={eps:g} drm10", r10, w10, v10))
            rows.append(value_row("drm_ratio", f"{n}x{h}x{w} eps={eps:g} drm12", r12, w12, v12))
    for i, (h, w) in enumerate(((37, 53), BIG_MAP)):
        d = torch.rand(1, 1, h, w, generator=torch.Generator().manual_seed(1820 + i))
        d[0, 0, 0, :4] = torch.tensor([0.0, 1.0, 0.5, float("nan")])
        for t in (0.2, 0.5, 0.8) if i == 0 else (0.3,):
            rows.append(exact_row("drm_retime", f"{h}x{w} t={t}", ops.drm_retime(d.to(dev), t), odrm.drm_to_t(d, t)))
    return rows


# ----------------------------------------------------------------------------------------- metric_input
METRIC_CASES = ((37, 53, 6.0), (64, 96, 12.0), (135, 240, 12.0))
UNSTABLE_CAP = 0.005
CLASS_MIN = 0.10


def metric_inputs(h, w, amp, seed):
    img0, img1 = _smooth(3, h, w, seed), _smooth(3, h, w, seed + 1)
    f01 = (_smooth(2, h, w, seed + 2) - 0.5) * amp
    f10 = -f01 + (_smooth(2, h, w, seed + 3) - 0.5) * 1.5  # nearly the inverse flow: the consistency test is undecided a priori
    return img0, img1, f01, f10


def fb_margins(fwd, bwd, alpha=0.01, beta=0.5):
    """geometry.py:87-108 (oracle.gmfss.fb_consistency) up to the comparison: d - thr per pixel, forward and backward."""
    mag = torch.norm(fwd, dim=1) + torch.norm(bwd, dim=1)
    d_f = torch.norm(fwd + ogm.flow_warp(bwd, fwd), dim=1)
    d_b = torch.norm(bwd + ogm.flow_warp(fwd, bwd), dim=1)
    thr = alpha * mag + beta
    return d_f - thr, d_b - thr


def metric_values_ref(img0, img1, f01, f10):
    """channels 0-11 of MetricNet's input (model_gmfss_union/MetricNet.py:45-60, oracle/gmfss.py:43-48)"""
    m0 = F.l1_loss(img0, backwarp_ref(img1, f01, "zeros"), reduction="none").mean([1], True)
    m1 = F.l1_loss(img1, backwarp_ref(img0, f10, "zeros"), reduction="none").mean([1], True)
    h, w = f01.shape[2:]
    nf = lambda f: torch.cat([f[:, 0:1] / ((w - 1.0) / 2.0), f[:, 1:2] / ((h - 1.0) / 2.0)], 1)  # noqa: E731
    return torch.cat((img0, img1, -m0, -m1, nf(f01), nf(f10)), 1)


def check_metric_input(dev, ops=None):
    ops = ops or default_ops()
    op, rows = "metric_input", []
    for i, (h, w, amp) in enumerate(METRIC_CASES):
        img0, img1, f01, f10 = metric_inputs(h, w, amp, 1900 + 10 * i)
        got = ops.metric_input(img0.to(dev), img1.to(dev), f01.to(dev), f10.to(dev)).detach().cpu()
        rows.append(value_row(op, f"{h}x{w} channels 0-11", got[:, :12], metric_values_ref(img0.double(), img1.double(), f01.double(), f10.double()),
                              metric_values_ref(img0, img1, f01, f10)))
        m64 = fb_margins(f01.double(), f10.double())
        m32 = fb_margins(f01, f10)
        for ch, name, a, b in ((12, "fwd_occ", m64[0], m32[0]), (13, "bwd_occ", m64[1], m32[1])):
            band = 4.0 * float((b.double() - a).abs().max())  # how far an fp32 evaluation of the margin strays, x 4
            ref, stable = a > 0, a.abs() > band
            ones, n_st = int((ref & stable).sum()), int(stable.sum())
            share = min(ones, n_st - ones) / max(n_st, 1)
            assert share >= CLASS_MIN, f"{name} {h}x{w}: {ones}/{n_st} stable ones: the input no longer exercises both classes"
            mask = got[:, ch]
            wrong = int(((mask != ref.float()) & stable).sum()) + int(((mask != 0) & (mask != 1)).sum())
            unstable = 1.0 - n_st / stable.numel()
            extra = f"band={band:.2e} ones={ones / max(n_st, 1):.1%} of {n_st} stable pixels"
            rows.append(Row(op, f"{h}x{w} {name} wrong stable decisions", float(wrong), 0.0, extra))
            rows.append(Row(op, f"{h}x{w} {name} unstable share", unstable, UNSTABLE_CAP, f"band={band:.2e} cap={UNSTABLE_CAP:.1%}"))
    return rows


# ----------------------------------------------------------------------------------------- softsplat
# The generic forward splat (drba_softsplat, _index, _again, _gather_quad: count, three-kernel scan, fill, optional segment sort,
# two gathers) against softsplat.py:248-367 / softsplat_torch.py:19-179 as oracle/ops.py restates them.
SPLAT_MODES = ("sum", "avg", "linear", "soft")
SPLAT_MAP = (37, 83)      # partial 32 x 8 tiles on both axes
SPLAT_BIG = (1024, 1280)  # 1 313 025 keys: scan_sums goes round more than once, the count / fill grid-stride loops 2.5 times
SPLAT_CHANNELS = (1, 2, 3, 15, 16, 17, 20, 32, 36, 64)  # both sides of the 16-channel chunk, quad (C >= 16, C % 4 == 0) and planar tails
SCAN_CASES = ((1, 63, 63), (2, 63, 63), (1, 63, 64), (3, 63, 64), (3,) + SPLAT_MAP)  # (N, H, W) of the scan-geometry rows
_SPLAT_REFS = {}  # row name -> (fp64 reference, fp32 oracle, the inputs they were computed from): once per process, never written to


def splat_keys(n, h, w):
    """entries of the key grid the sources are sorted on: footprints start anywhere in (-1 .. W-1) x (-1 .. H-1) of every image"""
    return n * (h + 1) * (w + 1)


def _grid32(h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys])


def splat_segment_sizes(flow):
    """how many sources share each footprint origin (floor of the fp32 target) that has any: the segment lengths of the index"""
    n, _, h, w = flow.shape
    t = (_grid32(h, w) + flow).floor()
    ok = torch.isfinite(t).all(1) & (t[:, 0] >= -1) & (t[:, 0] <= w - 1) & (t[:, 1] >= -1) & (t[:, 1] <= h - 1)
    key = (torch.arange(n).view(n, 1, 1) * (h + 1) + t[:, 1] + 1) * (w + 1) + t[:, 0] + 1
    return torch.bincount(key[ok].long())


def softsplat_ref(x, flow, metric, mode, dtype=torch.float64):
    """oracle.ops.softsplat in `dtype` on the targets the specification defines: X = x + flow is an fp32 sum (its first rounding,
    and what decides which four pixels a source lands on); weights, products, sums and the normalisation are then evaluated in
    `dtype`.  For float64 the flow handed to the dtype-generic oracle is X - x, exact in fp64, so that x + flow gives X back.
    Written out, because the oracle's int cast is not the specification there: a finite target beyond the int32 range has no
    corner inside the image (the reference's (int) saturates), so its source is skipped like one with a non-finite target."""
    _, _, h, w = flow.shape
    g = _grid32(h, w)
    t = g + flow
    far = t.abs() > 2.0 ** 30
    if dtype == torch.float32:
        f = torch.where(far, torch.full_like(flow, float("inf")), flow)
    else:
        t = torch.where(far, torch.full_like(t, float("inf")), t)
        f = t.to(dtype) - g.to(dtype)
        fin = torch.isfinite(t)
        assert torch.equal((g.to(dtype) + f)[fin], t.to(dtype)[fin])
    return oops.softsplat(x.to(dtype), f, None if metric is None else metric.to(dtype), mode)


def splat_refs(name, x, flow, metric, mode):
    """(fp64 reference, fp32 oracle) of a row, computed at its first use; a later use of the name must bring the same inputs"""
    ins = (x, flow, metric)
    if name not in _SPLAT_REFS:
        _SPLAT_REFS[name] = (softsplat_ref(x, flow, metric, mode), softsplat_ref(x, flow, metric, mode, torch.float32),
                             tuple(None if t is None else t.clone() for t in ins))
    for was, now in zip(_SPLAT_REFS[name][2], ins):
        assert (was is None and now is None) or (was is not None and now is not None and _mismatches(now, was) == 0), name
    return _SPLAT_REFS[name][:2]


def _splat_row(rows, ops, dev, name, x, flow, metric, mode, extra="", run=None):
    """one value row of ops.softsplat(x, flow, metric, mode), or of run(x, flow, metric) on the device tensors"""
    ref64, ref32 = splat_refs(f"{mode} {name}", x, flow, metric, mode)
    xd, fd, md = x.to(dev), flow.to(dev), None if metric is None else metric.to(dev)
    got = ops.softsplat(xd, fd, md, mode) if run is None else run(xd, fd, md)
    rows.append(value_row("softsplat", f"{mode} {name}", got, ref64, ref32, extra))


def splat_inputs(n, c, h, w, seed, mode="sum", sigma=2.0, positive=False):
    """x, flow, metric of a well-conditioned row: same-sign metrics where the metric is the weight itself (linear)"""
    x = torch.rand(n, c, h, w, generator=torch.Generator().manual_seed(seed)) + 0.5 if positive else cases.rnd((n, c, h, w), seed, 1.0)
    flow = cases.rnd((n, 2, h, w), seed + 1, sigma)
    metric = None
    if mode.startswith("linear"):
        metric = cases.rnd((n, 1, h, w), seed + 2, 1.0).abs() + 0.1
    elif mode.startswith("soft"):
        metric = cases.rnd((n, 1, h, w), seed + 2, 1.0)
    return x, flow, metric


def _f32_next(v, towards):
    return float(torch.nextafter(torch.tensor(float(v)), torch.tensor(float(towards))))


def border_flow(h, w, seed, alone=False):
    """[1, 2, h, w]: sigma = 2 noise, and sources whose targets are constructed (and asserted, as the fp32 sums they are):
    column 0 walks X over an integer, -1, its two fp32 neighbours, (-1, 0), W-1, (W-1, W), W, its lower neighbour, below -1 and
    above W (x = 0: the sum is the flow itself); row 0 does the same for Y; a 4 x 4 block takes every combination of
    {-1, -0.5, last, last + 0.5} on the two axes (the four corners of the image among them); source (0, 0) lands on the upper
    neighbours of (-1, -1); a few targets sit exactly on interior integers.
    alone=True: every other source leaves the image and the walks take every second row / column, so that a constructed source is
    the only one on its pixels -- under avg-zeroeps such a pixel is the source's value whatever the weight (2^-24 next to -1), and
    0 if the footprint is lost."""
    f = torch.full((1, 2, h, w), 1e4) if alone else cases.rnd((1, 2, h, w), seed, 2.0)
    step = 2 if alone else 1

    def walk(size):
        return [5.0, -1.0, _f32_next(-1, 0), _f32_next(-1, -2), -0.5, size - 1.0, size - 0.5, float(size), _f32_next(size, 0), -1.5, -40.0,
                size + 0.5, size + 40.0]

    want = {(0, 0): (_f32_next(-1, 0), _f32_next(-1, 0))}  # (y, x) of the source -> its target (X, Y)
    for k, t in enumerate(walk(w)):
        want[(step * k + 2, 0)] = (t, step * k + 2 + 0.25)
    for k, t in enumerate(walk(h)):
        want[(0, step * k + 2)] = (step * k + 2 + 0.25, t)
    for i, cx in enumerate((-1.0, -0.5, w - 1.0, w - 0.5)):
        for j, cy in enumerate((-1.0, -0.5, h - 1.0, h - 0.5)):
            want[(20 + j, 20 + i)] = (cx, cy)
    want[(30, 30)], want[(30, 31)], want[(31, 30)] = (12.0, 7.0), (0.0, 0.0), (w - 1.0, h - 1.0)
    for (y, x), (tx, ty) in want.items():
        f[0, 0, y, x], f[0, 1, y, x] = tx - x, ty - y
    t = _grid32(h, w) + f[0]
    for (y, x), (tx, ty) in want.items():
        assert float(t[0, y, x]) == float(torch.tensor(tx)) and float(t[1, y, x]) == float(torch.tensor(ty)), (y, x, tx, ty)
    return f


def nonfinite_flow(h, w, seed):
    """sigma = 2 noise with +-inf, NaN and +-1e30 in either component (and in both): none of these sources contributes"""
    f = cases.rnd((1, 2, h, w), seed, 2.0)
    inf, nan = float("inf"), float("nan")
    for k, (u, v) in enumerate(((inf, 0.3), (0.3, -inf), (nan, 0.3), (0.3, nan), (1e30, 0.3), (0.3, -1e30), (-1e30, 1e30), (inf, nan), (-inf, inf))):
        f[0, 0, 3 + 2 * k, 4 + 5 * k], f[0, 1, 3 + 2 * k, 4 + 5 * k] = u, v
    return f


def small_normaliser_inputs(seed):
    """Positive inputs, a flow that leaves the first columns uncovered (holes: normaliser exactly 0), and soft metrics around -12
    in the left half (normaliser ~ 6e-6: addeps' 1e-7 is 1.6 % of it, clipeps' bound below it) and around -20 in the right half
    (normaliser ~ 2e-9: clipeps divides by 1e-7 instead).  Same-sign weights: every quotient is well conditioned."""
    h, w = SPLAT_MAP
    x, flow, _ = splat_inputs(1, 3, h, w, seed, sigma=1.0, positive=True)
    flow[:, 0] += 6.3
    metric = cases.rnd((1, 1, h, w), seed + 2, 0.3) - 12.0
    metric[..., w // 2:] -= 8.0
    return x, flow, metric


ONTO = (41.25, 17.5)  # dyadic: the four weights are 0.375, 0.125, 0.375, 0.125, exact in fp32


def onto_flow(h, w):
    """every source of an h x w map onto ONTO: one segment of h * w records"""
    g = _grid32(h, w)
    return torch.stack([ONTO[0] - g[0], ONTO[1] - g[1]])[None].contiguous()


def onto_inputs(c, h, w, seed):
    """Positive inputs in [0.5, 1.5) on the 2^-6 grid.  With ONTO's weights every product is a multiple of 2^-9 below 0.6, and a
    sum of h * w = 3071 of them stays below 2^11: at most 20 bits, so every fp32 partial sum is exact in any order, and so is
    the normaliser.  What is left of the fp32 floor is avg's one division (and its 1e-7), so the rule's first term governs:
    2e-5 * |ref|max ~ 2e-5 * 3071 * 0.375 = 0.023 for sum, below the 0.0625 = 0.5 * 0.125 that one lost or doubled record is
    worth at the least."""
    return 0.5 + torch.floor(torch.rand(1, c, h, w, generator=torch.Generator().manual_seed(seed)) * 64.0) / 64.0


def zoom_flow(h, w):
    """zoom-out by 5 about the centre, fractional targets: 25 sources start their footprint at every pixel they reach"""
    g = _grid32(h, w)
    return torch.stack([-0.8 * (g[0] - w / 2 + 0.3), -0.8 * (g[1] - h / 2 + 0.2)])[None].contiguous()


REUSE_ROW = "soft softsplat_many reuse_index=True C=17 N=2 %dx%d" % SPLAT_MAP


def many_inputs():
    """inputs of C = 3, 64 and 17 (the largest is not the first) for one soft index at N = 2"""
    h, w = SPLAT_MAP
    xs = [splat_inputs(2, c, h, w, 2220 + k, positive=True)[0] for k, c in enumerate((3, 64, 17))]
    _, flow, metric = splat_inputs(2, 1, h, w, 2230, "soft")
    return xs, flow, metric


def _variants_differ(rows_tol, x, flow, metric, main, sub):
    """the fp64 references of the three eps variants on this input: the one under test is at least 100 tolerances from the others"""
    mine = softsplat_ref(x, flow, metric, f"{main}-{sub}")
    for other in ("addeps", "zeroeps", "clipeps"):
        if other != sub:
            d = (softsplat_ref(x, flow, metric, f"{main}-{other}") - mine).abs()
            assert float(d[torch.isfinite(d)].max()) > 100.0 * rows_tol, (main, sub, other)


def check_softsplat(dev, ops=None):
    """Borders, non-finite values, degenerate and partial-tile shapes, N > 1, the channel tails of both gathers, the three
    normalisers where they differ, many-to-one segments and every calling path, at 37 x 83 and below."""
    ops = ops or default_ops()
    rows = []
    h, w = SPLAT_MAP
    # ---- borders: constructed targets, every mode that has a normaliser of its own
    bf = border_flow(h, w, 2000)
    for k, mode in enumerate(("sum", "avg", "soft")):
        x, _, metric = splat_inputs(1, 3, h, w, 2010 + 3 * k, mode)
        _splat_row(rows, ops, dev, f"borders C=3 {h}x{w}", x, bf, metric, mode)
    alone = border_flow(h, w, 2000, alone=True)
    for mode in ("sum", "avg-zeroeps"):
        _splat_row(rows, ops, dev, f"borders, every other source outside, C=3 {h}x{w}", torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(2005)) + 0.5,
                   alone, None, mode)
    nf = nonfinite_flow(h, w, 2020)
    for k, mode in enumerate(("sum", "avg")):
        x, _, metric = splat_inputs(1, 3, h, w, 2030 + 3 * k, mode)
        _splat_row(rows, ops, dev, f"flow +-inf NaN +-1e30 C=3 {h}x{w}", x, nf, metric, mode)
    inf, nan = float("inf"), float("nan")
    for k, mode in enumerate(("avg", "linear", "soft")):
        x, flow, metric = splat_inputs(1, 3, h, w, 2040 + 3 * k, mode)
        x[0, 1, 12, 12], x[0, 0, 15, 15], x[0, 2, 18, 40] = nan, inf, -inf
        if metric is not None:
            metric[0, 0, 5, 5], metric[0, 0, 9, 9], metric[0, 0, 25, 60] = nan, inf, (-inf if mode == "soft" else 0.0)
        _splat_row(rows, ops, dev, f"NaN and inf in input and metric C=3 {h}x{w}", x, flow, metric, mode)
    # ---- shapes: one pixel, one row, one column; N = 3 of partial tiles
    one = torch.tensor([[0.0, 0.0], [-0.5, -0.25], [0.5, 0.5]]).view(3, 2, 1, 1)
    for mode in ("sum", "avg"):
        _splat_row(rows, ops, dev, "N=3 C=2 1x1", cases.rnd((3, 2, 1, 1), 2050, 1.0), one, None, mode)
    x, flow, metric = splat_inputs(1, 3, 1, w, 2053, "soft")
    flow[:, 1] *= 0.3
    _splat_row(rows, ops, dev, f"C=3 1x{w}", x, flow, metric, "soft")
    x, flow, metric = splat_inputs(2, 3, h, 1, 2056, "linear")
    flow[:, 0] *= 0.3
    _splat_row(rows, ops, dev, f"N=2 C=3 {h}x1", x, flow, metric, "linear")
    for k, mode in enumerate(SPLAT_MODES):
        x, flow, metric = splat_inputs(3, 5, h, w, 2060 + 3 * k, mode)
        _splat_row(rows, ops, dev, f"N=3 C=5 {h}x{w}", x, flow, metric, mode)
    # ---- channels: every count with two of the four modes, every mode with five counts, N = 2; the quad tails under linear and
    # soft (C = 20) and sum and avg (C = 36), the planar tail (C = 17) under avg and linear, and under sum by a row of its own
    for k, c in enumerate(SPLAT_CHANNELS):
        for mode in (SPLAT_MODES[k % 4], SPLAT_MODES[(k + 1) % 4]) + (("sum",) if c == 17 else ()):
            x, flow, metric = splat_inputs(2, c, h, w, 2100 + 3 * k, mode)
            _splat_row(rows, ops, dev, f"N=2 C={c} {h}x{w}", x, flow, metric, mode)
    # ---- normalisers: inputs on which the three eps variants give three answers
    x, flow, metric = small_normaliser_inputs(2200)
    holes = int((softsplat_ref(torch.ones(1, 1, h, w), flow, None, "sum") == 0).sum())
    assert holes > 0
    for sub in ("zeroeps", "clipeps", "addeps"):
        _splat_row(rows, ops, dev, f"normaliser 6e-6 | 2e-9, {holes} holes", x, flow, metric, f"soft-{sub}")
        _variants_differ(rows[-1][2], x, flow, metric, "soft", sub)
    neg = -3e-6 * (1.0 + 0.3 * torch.rand(1, 1, h, w, generator=torch.Generator().manual_seed(2203)))
    for sub in ("clipeps", "zeroeps"):  # (addeps on this input divides by ~0 where the normaliser is near -1e-7: no row)
        _splat_row(rows, ops, dev, f"all-negative metric ~-3e-6, {holes} holes", x, flow, neg, f"linear-{sub}")
        _variants_differ(rows[-1][2], x, flow, neg, "linear", sub)
    for sub in ("addeps", "zeroeps", "clipeps"):
        _splat_row(rows, ops, dev, f"C=3 {h}x{w}, {holes} holes", x, flow, None, f"avg-{sub}")
    # ---- many sources on one pixel
    ci = cases.ops_inputs()
    _splat_row(rows, ops, dev, "zoom-out x0.25 C=16 48x80", ci["x16"], ci["flow_converge"], ci["metric"], "soft")
    _splat_row(rows, ops, dev, "zoom-out x0.25 C=3 48x80", ci["x3"], ci["flow_converge"], None, "sum")
    x, _, metric = splat_inputs(1, 3, h, w, 2213, "linear")
    _splat_row(rows, ops, dev, f"zoom-out x0.2 C=3 {h}x{w}", x, zoom_flow(h, w), metric, "linear", "segments of 25 records")
    x, onto = onto_inputs(2, h, w, 2210), onto_flow(h, w)
    for mode in ("sum", "avg"):
        _splat_row(rows, ops, dev, f"every source onto {ONTO} C=2 {h}x{w}", x, onto, None, mode, f"one segment of {h * w} records")
    # ---- calling paths
    xs, flow, metric = many_inputs()
    fd, md = flow.to(dev), metric.to(dev)
    outs = ops.softsplat_many([x.to(dev) for x in xs], fd, md, "soft")
    for x, got in zip(xs, outs):
        name = f"soft softsplat_many [3, 64, 17] C={x.shape[1]} N=2 {h}x{w}"
        rows.append(value_row("softsplat", name, got, *splat_refs(name, x, flow, metric, "soft")))
    # (fd, md: the tensors the index was built from.  The values do not tell a reused index from a rebuilt one; that only the
    # gather is launched is asserted from the kernel trace, test_gpu_op_parity.py::test_softsplat_reuse_index_launches_one_gather)
    got = ops.softsplat_many([xs[2].to(dev)], fd, md, "soft", reuse_index=True)[0]
    rows.append(value_row("softsplat", REUSE_ROW, got, *splat_refs(REUSE_ROW, xs[2], flow, metric, "soft")))
    x, flow, metric = splat_inputs(2, 20, h, w, 2240, "linear")
    _splat_row(rows, ops, dev, f"keep_quad=True N=2 C=20 {h}x{w}", x, flow, metric, "linear", run=lambda a, f, m: ops.softsplat(a, f, m, "linear", keep_quad=True))
    x, flow, _ = splat_inputs(1, 3, h, w, 2250)
    buf = torch.full((1, 6, h, w), -7.25).to(dev)

    def into_slice(a, f, m):
        ops.softsplat(a, f, m, "avg", out=buf[:, 2:5])
        return buf[:, 2:5]  # (what the buffer holds, not what the call returned)

    _splat_row(rows, ops, dev, f"out= channels 2-4 of [1, 6, {h}, {w}]", x, flow, None, "avg", run=into_slice)
    rows.append(exact_row("softsplat", "out= channels 2-4: the rest of the buffer", buf[:, (0, 1, 5)], torch.full((1, 3, h, w), -7.25)))
    return rows


def check_softsplat_scan(dev, ops=None):
    """Scan geometry: one full block, two blocks, a ragged second block, image boundaries inside a scan block."""
    ops = ops or default_ops()
    rows = []
    for k, (n, h, w) in enumerate(SCAN_CASES):
        keys = splat_keys(n, h, w)
        for mode in (SPLAT_MODES[k % 4], SPLAT_MODES[(k + 1) % 4]):
            x, flow, metric = splat_inputs(n, 3, h, w, 2300 + 3 * k, mode)
            _splat_row(rows, ops, dev, f"N={n} C=3 {h}x{w}", x, flow, metric, mode, f"keys={keys}")
    return rows


def check_softsplat_big(dev, ops=None):
    """One map past every single-round bound of the index: 1 313 025 keys, sigma = 6 flow."""
    ops = ops or default_ops()
    rows = []
    h, w = SPLAT_BIG
    for k, (c, mode) in enumerate(((3, "avg"), (2, "soft"))):
        x, flow, metric = splat_inputs(1, c, h, w, 2400 + 3 * k, mode, sigma=6.0)
        _splat_row(rows, ops, dev, f"C={c} {h}x{w}", x, flow, metric, mode, f"keys={splat_keys(1, h, w)}")
    return rows


# ----------------------------------------------------------------------------------------- resize_bilinear_scale
RESIZE_SCALE_CASES = ((2, 3, 37, 53, 0.5), (1, 2, 45, 83, 0.25), (1, 3, 13, 45, 2.0), (2, 2, 4, 5, 0.25), (1, 3) + BIG_MAP + (0.5,))


def resize_scale_ref(x, factor):
    """F.interpolate(x, scale_factor=factor, mode="bilinear", align_corners=False) written out (GMFSS.py's _half, IFNet's
    stage inputs): out size floor(in * factor); the source coordinate of output i is max((i + 0.5) / factor - 0.5, 0) -- the
    multiplier is 1 / factor as given, not the ratio of the sizes --, taps i0 = min(floor(s), in - 1) and min(i0 + 1, in - 1)."""
    def axis(n_in):
        n_out = int(n_in * factor)
        s = ((torch.arange(n_out, dtype=x.dtype) + 0.5) * (1.0 / factor) - 0.5).clamp(min=0.0)
        i0 = s.floor().clamp(max=n_in - 1)
        return i0.long(), (i0 + 1).clamp(max=n_in - 1).long(), s - i0

    y0, y1, ly = axis(x.shape[2])
    x0, x1, lx = axis(x.shape[3])
    ly = ly.view(-1, 1)
    top = x[:, :, y0][:, :, :, x0] * (1 - lx) + x[:, :, y0][:, :, :, x1] * lx
    bot = x[:, :, y1][:, :, :, x0] * (1 - lx) + x[:, :, y1][:, :, :, x1] * lx
    return top * (1 - ly) + bot * ly


def check_resize_scale(dev, ops=None):
    ops = ops or default_ops()
    rows = []
    for i, (n, c, h, w, s) in enumerate(RESIZE_SCALE_CASES):
        x = cases.rnd((n, c, h, w), 2500 + i, 2.0)
        ho, wo = int(h * s), int(w * s)
        got = ops.resize_bilinear_scale(x.to(dev), (ho, wo), 1.0 / s)
        rows.append(value_row("resize_bilinear_scale", f"[{n}x{c}] {h}x{w} x{s:g} -> {ho}x{wo}", got, resize_scale_ref(x.double(), s),
                              F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False)))
    return rows


# ----------------------------------------------------------------------------------------- flow_distance
def flow_distance_ref(flow):
    """tools.py:77-80: sqrt(u^2 + v^2), computed by the reference in fp32 -- so where the fp32 squares (or their sum) overflow
    the specified answer is +inf, whatever the exact magnitude; everywhere else the exact value in fp64."""
    u, v = flow[:, 0:1], flow[:, 1:2]
    d = torch.sqrt(u.double() ** 2 + v.double() ** 2)
    over = torch.isinf(u.float() ** 2 + v.float() ** 2)
    return torch.where(over, torch.full_like(d, float("inf")), d)


def check_flow_distance(dev, ops=None):
    ops = ops or default_ops()
    rows = []
    for i, shape in enumerate(((2, 2, 13, 45), (1, 2) + BIG_MAP)):
        f = cases.rnd(shape, 2600 + i, 5.0)
        rows.append(value_row("flow_distance", f"{list(shape)}", ops.flow_distance(f.to(dev)), flow_distance_ref(f), oops.distance(f)))
    inf, nan = float("inf"), float("nan")
    u = torch.tensor([0.0, -0.0, 1e-40, 3.0, nan, 1.0, inf, -inf, inf, 2e19, -1.5e19, 1e30, 1e-20, -0.0])
    v = torch.tensor([-0.0, 0.0, 0.0, -4.0, 1.0, nan, 1.0, 2.0, nan, 0.0, 1.5e19, -1e30, 1e-20, 5.0])
    f = torch.stack([u, v]).view(1, 2, 1, -1)
    rows.append(value_row("flow_distance", "+-0, denormal, NaN, +-inf, squares that overflow fp32", ops.flow_distance(f.to(dev)), flow_distance_ref(f),
                          oops.distance(f)))
    return rows


# ----------------------------------------------------------------------------------------- IFNet stage glue
# ifnet_glue.hip, flow_terms.hpp, stage_conv.hip, stage_conv16.hip in the forms the pipeline runs: frames read from their
# [H, W, 4] copies (ops.rgbx), pair-only features, the running flow as terms (one-row term maps among them), the fused
# first convolution at scale 1 and 2, the final blend at the frame's own resolution with four terms.  References from
# IFNet_HDv3.py:85-95 (IFBlock.forward) and :146-167 (the stage loop and the final blend).
STAGE_GROUPS = (("frames", 0, 6), ("features", 6, 38), ("timestep", 38, 39), ("mask/feat", 39, 48), ("flow", 48, 52))
T_SCALAR = 0.37


def up(t, s):
    return F.interpolate(t, scale_factor=float(s), mode="bilinear", align_corners=False)


def _down(x, s):
    """F.interpolate(x, scale_factor=1 / s) (IFNet_HDv3.py:85,87).  At s = 1 it is the identity, and written as one: ATen forms
    t0 + 0 * (t1 - t0) there, NaN at a non-finite pixel (its CUDA kernel: 1 * t0 + 0 * t1, NaN at the neighbour instead), which is
    not the specification of a resize by 1."""
    return x if s == 1 else F.interpolate(x, scale_factor=1.0 / s, mode="bilinear", align_corners=False)


def running_flow(terms, tmp_prev, sp):
    """IFNet_HDv3.py:146-160: sum of up(t_i[:, :4], s_i) * s_i over the earlier head outputs (oldest first, possibly none) and the
    newest one, tmp_prev at scale sp."""
    fl = None
    for t, s in list(terms) + [(tmp_prev, sp)]:
        d = up(t[:, :4], s) * s
        fl = d if fl is None else fl + d
    return fl


def update_ref(tmp, flow_in, s):
    """IFNet_HDv3.py:92-95,160 -> (flow_in + up(tmp[:, :4]) * s, mask, feat)"""
    u = up(tmp, s)
    fd = u[:, :4] * s
    return (fd if flow_in is None else flow_in + fd), u[:, 4:5], u[:, 5:13]


def stage_input_ref(img0, img1, f0, f1, timestep, flow, tmp_prev, sp, s):
    """IFNet_HDv3.py:85-95,151-156: the IFBlock's input at 1 / s.  flow None: the first stage's 39 channels."""
    tmap = timestep if torch.is_tensor(timestep) else torch.full_like(img0[:, :1], float(timestep))
    if flow is None:
        return _down(torch.cat((img0, img1, f0, f1, tmap), 1), s)
    u = up(tmp_prev, sp)
    warp = lambda x, f: backwarp_ref(x, f, "border")  # noqa: E731
    x = torch.cat((warp(img0, flow[:, :2]), warp(img1, flow[:, 2:4]), warp(f0, flow[:, :2]), warp(f1, flow[:, 2:4]), tmap, u[:, 4:5], u[:, 5:13]), 1)
    return torch.cat((_down(x, s), _down(flow, s) * (1.0 / s)), 1)


def blend_ref(img0, img1, flow, mask_logit):
    """IFNet_HDv3.py:163-167"""
    m = torch.sigmoid(mask_logit)
    return backwarp_ref(img0, flow[:, :2], "border") * m + backwarp_ref(img1, flow[:, 2:4], "border") * (1 - m)


def stage_conv_ref(img0, img1, f0, f1, timestep, flow, tmp_prev, sp, s, w, b):
    """conv0[0] of the IFBlock (IFNet_HDv3.py:8-14,68) on its stage input"""
    return F.leaky_relu(F.conv2d(stage_input_ref(img0, img1, f0, f1, timestep, flow, tmp_prev, sp, s), w, b, stride=2, padding=1), 0.2)


def _fold_input_ref(img0, img1, f0, f1, timestep, prior, tmp_prev, sp, s):
    return stage_input_ref(img0, img1, f0, f1, timestep, update_ref(tmp_prev, prior, sp)[0], tmp_prev, sp, s)


def _lazy_input_ref(img0, img1, f0, f1, timestep, terms, tmp_prev, sp, s):
    return stage_input_ref(img0, img1, f0, f1, timestep, running_flow(terms, tmp_prev, sp), tmp_prev, sp, s)


def _cast(a, dt):
    if torch.is_tensor(a):
        return a.to(dt)
    if isinstance(a, (list, tuple)):
        return type(a)(_cast(b, dt) for b in a)
    return a


_GLUE_REFS = {}  # key -> (fp64 reference, fp32 form): computed once per process, never written to


def refs(fn, *args, key=None):
    """(fn in float64, fn in float32) on the same arguments: the reference and the floor of a row.  key: the name the pair is
    kept under (the inputs regenerate from seeds, so a key names one set of arguments)."""
    if key is None:
        return fn(*_cast(args, torch.float64)), fn(*_cast(args, torch.float32))
    if key not in _GLUE_REFS:
        _GLUE_REFS[key] = refs(fn, *args)
    return _GLUE_REFS[key]


def glue_frames(n, h, w, seed):
    """img0, img1 [n, 3, h, w] in [0, 1], f0, f1 [n, 16, h, w] of amplitude 4, a timestep map [n, 1, h, w]: smooth fields, so that
    the fp32 floor of a warped row (the coordinate's round trip through [-1, 1], a few ulps of W - 1, times the largest
    neighbour difference) stays below the rule's first term"""
    sm = lambda c, k: _smooth(n * c, h, w, seed + k).view(n, c, h, w)  # noqa: E731
    return sm(3, 0), sm(3, 1), (sm(16, 2) - 0.5) * 8.0, (sm(16, 3) - 0.5) * 8.0, sm(1, 4)


def glue_heads(n, h, w, scales, seed, rough=None):
    """{s: head output [n, 13, h / s, w / s]}: flow channels of amplitude 2 / s (the update up(t[:, :4]) * s is a few pixels per
    stage); rough=s: that term's update has sigma 4 w, so that most samples clamp at the border"""
    out = {}
    for s in scales:
        assert h % s == 0 and w % s == 0, (h, w, s)  # (the reference model cannot form other sizes)
        t = cases.rnd((n, 13, h // s, w // s), seed + s, 1.0)
        t[:, :4] *= 2.0 / s * (2.0 * w if s == rough else 1.0)
        out[s] = t
    return out


def flows4(h, w, seed):
    """name -> [1, 4, h, w] of warp_flows: channels 0-1 warp img0, 2-3 img1"""
    return {k: v.reshape(1, 4, h, w) for k, v in warp_flows(2, h, w, seed).items()}


def glue_item(dev, ops, fr, k, x4=False, pair=False, tscalar=None):
    """(img0, img1, timestep, f0, f1) of item k on the device, as tensors of its own: the layout copies live on the tensor object"""
    img0, img1, f0, f1, tm = (t[k:k + 1].clone().to(dev) for t in fr)
    if x4:
        ops.rgbx(img0), ops.rgbx(img1)
    if pair:
        f0, f1 = ops.pair_interleaved(f0), ops.pair_interleaved(f1)
    return (img0, img1, tm if tscalar is None else tscalar, f0, f1)


def stage_rows(op, name, got, ref64, ref32):
    """one row per channel group of a stage input, each with its own |ref|max and floor"""
    if got.dim() != 4 or got.shape[1] != ref64.shape[1]:
        return [Row(op, name, float("inf"), 0.0, f"shape {tuple(got.shape)} for {tuple(ref64.shape)}")]
    return [value_row(op, f"{name} {g}", got[:, a:b], ref64[:, a:b], ref32[:, a:b]) for g, a, b in STAGE_GROUPS if b <= ref64.shape[1]]


def _scalar_t(r):
    """the references of the same row with the scalar timestep: a constant map stays the constant under the downsample"""
    out = []
    for t in r:
        t = t.clone()
        t[:, 38] = T_SCALAR
        out.append(t)
    return out


FIRST_CASES = (((64, 128), (16, 4, 1)), ((72, 136), (4, 2, 1)), ((70, 90), (1,)))


def check_stage_input_first(dev, ops=None):
    """The first stage (no flow, 39 channels): ifblock_input_pixel / ifblock_input_kernel<false, ...>, planar and pair-only features."""
    ops = ops or default_ops()
    rows = []
    for i, ((h, w), scales) in enumerate(FIRST_CASES):
        fr = glue_frames(1, h, w, 3000 + 10 * i)
        for s in scales:
            r = refs(stage_input_ref, *fr, None, None, 1.0, s, key=f"first {h}x{w} s={s}")
            for tscalar in (None, T_SCALAR):
                rr = r if tscalar is None else _scalar_t(r)
                for pair in (False, True):
                    it = glue_item(dev, ops, fr, 0, pair=pair, tscalar=tscalar)
                    got = ops.ifblock_input(it[0], it[1], it[3], it[4], it[2], None, None, 1.0, s)
                    name = f"first {h}x{w} s={s} t={'map' if tscalar is None else 'scalar'} features={'pair-only' if pair else 'planar'}"
                    rows += stage_rows("ifblock_input", name, got, *rr)
    h, w, s = 72, 136, 2
    fr = glue_frames(3, h, w, 3050)
    items = [glue_item(dev, ops, fr, k, pair=True) for k in range(3)]
    out = torch.full((3, 39, h // s, w // s), float("nan")).to(dev)
    ops.stage_inputs(items, None, None, 1.0, s, out, lds=False)
    rows += stage_rows("stage_inputs", f"first B=3 {h}x{w} s={s} lds=False features=pair-only", out, *refs(stage_input_ref, *fr, None, None, 1.0, s, key="first B=3"))
    return rows


def _stage_inputs_out(ops, dev, items, flows, tp, sp, s, fold=False, terms=None):
    """ops.stage_inputs into a NaN-filled [B, 52, h / s, w / s] -> (out, the folded flows or None)"""
    h, w = items[0][0].shape[2:]
    out = torch.full((len(items), 52, h // s, w // s), float("nan")).to(dev)
    fo = ops.stage_inputs(items, flows, tp, float(sp), float(s), out, fold=fold, terms=terms)
    return out, fo


def check_stage_input_warped(dev, ops=None):
    """Warped stage inputs with the flow finished (FMODE 0), folded (1) and as terms (2); planar and [H, W, 4] frames."""
    ops = ops or default_ops()
    rows = []
    D = lambda t: t.to(dev)  # noqa: E731
    # ---- finished flow: whole tiles (vector stores) at 64 x 128, ragged tiles (scalar stores) at 72 x 136
    for i, ((h, w), scales) in enumerate((((64, 128), (8, 2, 1)), ((72, 136), (4, 2, 1)))):
        fr = glue_frames(1, h, w, 3100 + 10 * i)
        heads = glue_heads(1, h, w, [2 * s for s in scales], 3120 + 100 * i)
        for s in scales:
            sp, tp = 2 * s, heads[2 * s]
            for fname, flow in flows4(h, w, 3140 + 10 * i).items():
                tag = f"{h}x{w} s={s} {fname}"
                r = refs(stage_input_ref, *fr, flow, tp, float(sp), s, key="warped " + tag)
                it = glue_item(dev, ops, fr, 0)
                got = ops.ifblock_input(it[0], it[1], it[3], it[4], it[2], D(flow), D(tp), float(sp), float(s))
                rows += stage_rows("ifblock_input", f"warped {tag} t=map", got, *r)
                got = ops.ifblock_input_lds(it[0], it[1], it[3], it[4], T_SCALAR, D(flow), D(tp), float(sp), float(s))
                rows += stage_rows("ifblock_input_lds", f"{tag} t=scalar", got, *_scalar_t(r))
                if s <= 2:
                    got, _ = _stage_inputs_out(ops, dev, [glue_item(dev, ops, fr, 0, x4=True)], [D(flow)], D(tp), sp, s)
                    rows += stage_rows("stage_inputs", f"{tag} x4 t=map", got, *r)
    # ---- the previous stage's update folded in, with a prior flow (planar frames) and with none (x4 frames, the batched entry)
    for i, (h, w, s) in enumerate(((64, 128, 2), (64, 128, 1), (70, 90, 1), (72, 136, 2))):
        fr = glue_frames(1, h, w, 3200 + 10 * i)
        sp, tp = 2 * s, glue_heads(1, h, w, [2 * s], 3220 + 100 * i)[2 * s]
        prior = flows4(h, w, 3240 + 10 * i)["smooth"] * 0.5
        tag = f"fold {h}x{w} s={s}"
        it = glue_item(dev, ops, fr, 0)
        got, fo = ops.ifblock_input_lds(it[0], it[1], it[3], it[4], it[2], D(prior), D(tp), float(sp), float(s), fold=True)
        rows.append(value_row("ifblock_input_lds", f"{tag} prior flow: flow_out", fo, *refs(lambda t, f: update_ref(t, f, sp)[0], tp, prior, key=tag + " flow")))
        rows += stage_rows("ifblock_input_lds", f"{tag} prior flow", got, *refs(_fold_input_ref, *fr, prior, tp, float(sp), s, key=tag))
        got, fo = _stage_inputs_out(ops, dev, [glue_item(dev, ops, fr, 0, x4=True)], [None], D(tp), sp, s, fold=True)
        rows.append(value_row("stage_inputs", f"{tag} no prior flow x4: flow_out", fo[0], *refs(lambda t: update_ref(t, None, sp)[0], tp, key=tag + " flow, no prior")))
        rows += stage_rows("stage_inputs", f"{tag} no prior flow x4", got, *refs(_fold_input_ref, *fr, None, tp, float(sp), s, key=tag + ", no prior"))

    # ---- the flow as terms
    def lazy(n, h, w, s, tscales, seed, x4s, rough=None):
        fr = glue_frames(n, h, w, seed)
        sp = 2 * s
        heads = glue_heads(n, h, w, list(tscales) + [sp], seed + 20, rough)
        terms = [(heads[t], float(t)) for t in tscales]
        r = refs(_lazy_input_ref, *fr, terms, heads[sp], float(sp), s, key=f"lazy input {seed}")
        for x4 in x4s:
            items = [glue_item(dev, ops, fr, k, x4=x4) for k in range(n)]
            got, _ = _stage_inputs_out(ops, dev, items, None, D(heads[sp]), sp, s, terms=[(D(t), ts) for t, ts in terms])
            name = f"lazy {'B=%d ' % n if n > 1 else ''}{h}x{w} s={s} terms={tuple(tscales)}{' rough' if rough else ''} {'x4' if x4 else 'planar'}"
            rows.extend(stage_rows("stage_inputs", name, got, *r))

    lazy(1, 64, 128, 8, (), 3300, (False,))
    lazy(1, 64, 128, 4, (16,), 3310, (False,))
    lazy(1, 64, 128, 2, (16, 8), 3320, (False, True))
    lazy(1, 64, 128, 1, (16, 8, 4), 3330, (False, True))
    lazy(1, 16, 48, 1, (16, 8, 4), 3340, (True,))       # the oldest term map is 1 x 3
    lazy(3, 96, 160, 2, (16, 8), 3350, (True,))          # 12 tiles x 3 items
    lazy(1, 72, 136, 2, (8,), 3380, (True,))             # ragged tiles: four sample points per output, the scalar stores
    lazy(1, 64, 128, 1, (16, 8, 4), 3360, (True,), rough=16)
    lazy(1, 64, 128, 4, (16,), 3370, (False,), rough=16)
    return rows


def check_stage_conv_fused(dev, ops=None):
    """The stage input fused with conv0[0] (stage_conv.hip, stage_conv16.hip) against torch in fp64 end to end."""
    ops = ops or default_ops()
    rows = []
    D = lambda t: t.to(dev)  # noqa: E731
    was = getattr(ops, "STAGE_CONV_TWO_TERM", None)

    def conv_of(cout, seed):
        wt, bs = cases.rnd((cout, 52, 3, 3), seed, 1.0 / (52 * 9) ** 0.5), cases.rnd((cout,), seed + 1, 0.1)
        return wt, bs, ops.Conv3x3(wt, bs, 2, True, None, device=dev)

    def run(name, conv, items, h, w, s, sp, tp, ref, flows=None, fold=False, terms=None, flow_ref=None):
        assert ops.stage_conv0_ok(conv, h, w, float(s), float(sp), items=items), f"stage_conv0_ok refuses {name}"
        y, fo = ops.stage_conv0(items, flows, D(tp), float(sp), conv, fold=fold, terms=terms, scale=s)
        rows.append(value_row("stage_conv0", name, y, *ref))
        if fold:
            rows.append(value_row("stage_conv0", f"{name}: flow_out", fo[0], *flow_ref))

    try:
        for two in (True, False):
            ops.STAGE_CONV_TWO_TERM = two
            form = "two-term" if two else "fp32"
            for i, (h, w) in enumerate(((64, 128), (70, 90), (38, 66))):
                fr = glue_frames(1, h, w, 3400 + 10 * i)
                tscales = (16, 8, 4) if (h, w) == (64, 128) else ()  # (70 and 38 are multiples of 2 only: no earlier stage can exist)
                heads = glue_heads(1, h, w, tscales + (2,), 3420 + 100 * i)
                tp = heads[2]
                wt, bs, conv = conv_of(16, 3440 + 10 * i)
                flow = flows4(h, w, 3460 + 10 * i)["smooth"]
                for x4 in (True, False):
                    tag = f"{form} s=1 {h}x{w} {'x4' if x4 else 'planar'}"
                    item = lambda: [glue_item(dev, ops, fr, 0, x4=x4)]  # noqa: E731
                    run(f"{tag} finished flow", conv, item(), h, w, 1, 2, tp, refs(stage_conv_ref, *fr, flow, tp, 2.0, 1, wt, bs, key=f"conv {h}x{w} finished"),
                        flows=[D(flow)])
                    prior = flow * 0.5 if x4 else None
                    fref = refs(lambda t, f: update_ref(t, f, 2)[0], tp, prior, key=f"conv {h}x{w} fold flow {x4}")
                    run(f"{tag} fold, {'a' if x4 else 'no'} prior flow", conv, item(), h, w, 1, 2, tp,
                        refs(lambda *a: stage_conv_ref(*a[:5], update_ref(a[6], a[5], 2)[0], *a[6:]), *fr, prior, tp, 2.0, 1, wt, bs, key=f"conv {h}x{w} fold {x4}"),
                        flows=[None if prior is None else D(prior)], fold=True, flow_ref=fref)
                    terms = [(heads[t], float(t)) for t in tscales]
                    run(f"{tag} terms={tscales}", conv, item(), h, w, 1, 2, tp,
                        refs(lambda *a: stage_conv_ref(*a[:5], running_flow(a[5], a[6], 2.0), *a[6:]), *fr, terms, tp, 2.0, 1, wt, bs, key=f"conv {h}x{w} terms"),
                        terms=[(D(t), ts) for t, ts in terms])
        ops.STAGE_CONV_TWO_TERM = True  # scale 2: the two-term kernel only, lazy flow, x4 frames
        for i, (n, h, w, tscales) in enumerate(((1, 64, 128, (16, 8)), (1, 72, 104, (8,)), (3, 96, 160, (16, 8)))):
            fr = glue_frames(n, h, w, 3500 + 10 * i)
            heads = glue_heads(n, h, w, tscales + (4,), 3520 + 100 * i)
            terms = [(heads[t], float(t)) for t in tscales]
            for cout in (16, 32):
                wt, bs, conv = conv_of(cout, 3540 + 10 * i + cout)
                items = [glue_item(dev, ops, fr, k, x4=True) for k in range(n)]
                run(f"two-term s=2 cout={cout} {'B=%d ' % n if n > 1 else ''}{h}x{w} terms={tscales} x4", conv, items, h, w, 2, 4, heads[4],
                    refs(lambda *a: stage_conv_ref(*a[:5], running_flow(a[5], a[6], 4.0), *a[6:]), *fr, terms, heads[4], 4.0, 2, wt, bs,
                         key=f"conv s=2 {h}x{w} {cout}"),
                    terms=[(D(t), ts) for t, ts in terms])
    finally:
        ops.STAGE_CONV_TWO_TERM = was
    return rows


def check_flow_update(dev, ops=None):
    ops = ops or default_ops()
    rows = []
    D = lambda t: t.to(dev)  # noqa: E731
    for i, (h, w, s) in enumerate(((64, 128, 16), (64, 128, 2), (64, 128, 1), (70, 90, 2))):
        tmp = glue_heads(1, h, w, [s], 3600 + 100 * i)[s]
        flow = flows4(h, w, 3620 + 10 * i)["amp30"]
        tag = f"{h}x{w} s={s}"
        gf, gm, gfe = ops.ifblock_update(D(tmp), D(flow), h, w, float(s), want_mask_feat=True)
        r64, r32 = refs(update_ref, tmp, flow, s, key="update " + tag)
        rows.append(value_row("ifblock_update", f"{tag} flow", gf, r64[0], r32[0]))
        rows.append(value_row("ifblock_update", f"{tag} mask", gm, r64[1], r32[1]))
        rows.append(value_row("ifblock_update", f"{tag} feat", gfe, r64[2], r32[2]))
        rows.append(value_row("ifblock_update", f"{tag} no prior flow, no mask / feat", ops.ifblock_update(D(tmp), None, h, w, float(s)),
                              *refs(lambda t: update_ref(t, None, s)[0], tmp, key="update, no prior " + tag)))
    h, w, s = 64, 128, 2
    tmp = glue_heads(3, h, w, [s], 3700)[s]
    f1 = flows4(h, w, 3710)["smooth"]
    got = ops.flow_updates(D(tmp), [None, D(f1), None], h, w, float(s))
    for k, f in enumerate((None, f1, None)):
        rows.append(value_row("flow_updates", f"B=3 {h}x{w} s={s} item {k} ({'a' if f is not None else 'no'} prior flow)", got[k],
                              *refs(lambda t, p: update_ref(t, p, s)[0], tmp[k:k + 1], f, key=f"updates {k}")))
    return rows


def _blend_fold_ref(img0, img1, prior, tmp, s):
    fl, mask, _ = update_ref(tmp, prior, s)
    return blend_ref(img0, img1, fl, mask)


def _blend_lazy_ref(img0, img1, terms, tmp, s):
    return blend_ref(img0, img1, running_flow(terms, tmp, s), up(tmp, s)[:, 4:5])


def check_warp_blend(dev, ops=None):
    """The final warp + blend: flow finished, folded, and as terms -- at the frame's own resolution (S1) and staged."""
    ops = ops or default_ops()
    rows = []
    D = lambda t: t.to(dev)  # noqa: E731
    for i, (h, w, s) in enumerate(((37, 83, 1), (64, 128, 1), (64, 128, 2), (38, 66, 2))):
        fr = glue_frames(1, h, w, 3800 + 10 * i)
        tmp = glue_heads(1, h, w, [s], 3820 + 100 * i)[s]
        img0, img1 = D(fr[0]), D(fr[1])
        for fname, flow in flows4(h, w, 3840 + 10 * i).items():
            tag = f"{h}x{w} head s={s} {fname}"
            rows.append(value_row("warp_blend", tag, ops.warp_blend(img0, img1, D(flow), D(tmp), float(s)),
                                  *refs(lambda a, b, f, t: blend_ref(a, b, f, up(t, s)[:, 4:5]), fr[0], fr[1], flow, tmp, key="blend " + tag)))
            rows.append(value_row("warp_blend_fold", tag + " as prior flow", ops.warp_blend_fold(img0, img1, D(flow), D(tmp), float(s)),
                                  *refs(_blend_fold_ref, fr[0], fr[1], flow, tmp, s, key="blend fold " + tag)))
        rows.append(value_row("warp_blend_fold", f"{h}x{w} head s={s} no prior flow", ops.warp_blend_fold(img0, img1, None, D(tmp), float(s)),
                              *refs(_blend_fold_ref, fr[0], fr[1], None, tmp, s, key=f"blend fold {h}x{w} {s}, no prior")))
        if (h, w) == (64, 128):  # mask logits x 30: the sigmoid saturates both ways
            sat = tmp.clone()
            sat[:, 4] *= 30.0
            flow = flows4(h, w, 3840 + 10 * i)["smooth"]
            rows.append(value_row("warp_blend", f"{h}x{w} head s={s} smooth, saturating mask", ops.warp_blend(img0, img1, D(flow), D(sat), float(s)),
                                  *refs(lambda a, b, f, t: blend_ref(a, b, f, up(t, s)[:, 4:5]), fr[0], fr[1], flow, sat, key=f"blend saturating {s}")))

    def lazy(n, h, w, last, tscales, seed, x4s, rough=None):
        fr = glue_frames(n, h, w, seed)
        heads = glue_heads(n, h, w, list(tscales) + [last], seed + 20, rough)
        terms = [(heads[t], float(t)) for t in tscales]
        r = refs(_blend_lazy_ref, fr[0], fr[1], terms, heads[last], last, key=f"lazy blend {seed}")
        for x4 in x4s:
            items = [glue_item(dev, ops, fr, k, x4=x4)[:2] for k in range(n)]
            got = torch.cat(list(ops.warp_blend_lazy(items, [(D(t), ts) for t, ts in terms], D(heads[last]), float(last))))
            name = f"{'S1' if last == 1 else 'staged'} {'B=%d ' % n if n > 1 else ''}{h}x{w} last={last} terms={tuple(tscales)}{' rough' if rough else ''} " \
                   f"{'x4' if x4 else 'planar'}"
            rows.append(value_row("warp_blend_lazy", name, got, *r))

    lazy(1, 48, 80, 1, (16, 8, 4, 2), 3900, (False, True))   # 2.5 x 6 tiles
    lazy(1, 16, 48, 1, (16, 8, 4, 2), 3910, (False, True))   # the oldest term map is 1 x 3
    lazy(1, 38, 66, 1, (2,), 3920, (False, True))            # the term footprint under a 32 x 8 tile is the 18 x 6 capacity
    lazy(3, 48, 80, 1, (16, 8, 4, 2), 3930, (True,))
    lazy(1, 48, 80, 1, (16, 8, 4, 2), 3940, (True,), rough=16)
    lazy(1, 64, 128, 2, (32, 16, 8, 4), 3950, (False, True))  # the 4K half-scale configuration
    lazy(1, 48, 80, 2, (16, 8, 4), 3960, (False, True))
    return rows


# ----------------------------------------------------------------------------------------- conv epilogue forms
# Every configuration id of drba_conv3x3 carries its own copy of the epilogue (conv.hip, conv_split.hip, conv_dma.hip, conv_ks.hip):
# bias, y * beta + x or + residual (+ residual2), five activations, the PReLU pre-activation of the loader, vector and element-wise
# stores, and in three files an "RL" instantiation that rebuilds the residual from the input window when residual == in.  Each form
# a model constructs is run here with every id pinned (cfg=), against F.conv2d in float64 and the epilogue formula of
# include/drba_hip.h:432-438 written out.  Nothing is tuned or timed.
ConvForm = collections.namedtuple("ConvForm", "name layer bias act post_slope pre_slope cout res beta")
CONV_FORMS = (  # res: None, "in" (the input tensor itself), "other", "other2" (two other tensors), "same" / "copy" (ResConv, see below)
    ConvForm("plain", "ResidualBlock.c1/c2, trident (gmflow.py)", False, None, 0.0, None, None, None, False),
    ConvForm("bias+relu", "up0 (gmflow.py)", True, "relu", 0.0, None, None, None, False),
    ConvForm("bias+prelu(0.1)", "tail_a (FusionNet.py)", True, "prelu", 0.1, None, None, None, False),
    ConvForm("pre+tanh10 Cout=2", "conv_out (MetricNet.py)", True, "tanh10", 0.0, 0.25, 2, None, False),
    ConvForm("Cout=3", "tail_last (FusionNet.py)", True, None, 0.0, None, 3, None, False),
    ConvForm("bias+lrelu", "conv (IFNet_HDv3.py), as check_conv_layers", True, True, 0.0, None, None, None, False),
    ConvForm("pre", "FeatureNet / FusionNet convs, as check_conv_layers", True, None, 0.0, 0.25, None, None, False),
    ConvForm("pre+res=in", "mid[k] (MetricNet.py): residual=feat, the input itself, no beta", True, None, 0.0, 0.25, None, "in", False),
    ConvForm("pre+res+res2", "_TwoConv.second (FusionNet.py)", True, None, 0.0, 0.25, None, "other2", False),
    ConvForm("res", "one other-tensor residual", True, None, 0.0, None, None, "other", False),
    ConvForm("resconv res is in", "ResConv (IFNet_HDv3.py): residual= the same tensor object as the input", True, True, 0.0, None, None, "same", True),
    ConvForm("resconv res copy", "ResConv with a second copy of the input, as check_conv_layers", True, True, 0.0, None, None, "copy", True))
CONV_PLAIN_FORMS = tuple(f.name for f in CONV_FORMS if f.res is None)     # what a stride-2 id takes
CONV_RESIDUAL_FORMS = tuple(f.name for f in CONV_FORMS if f.res is not None)
CONV_MAPS = ((2, 11, 44), (1, 9, 45))  # (N, H, W): W % 4 == 0 with partial tiles on both axes; W % 4 != 0 (element-wise stores).  Guarded.
CONV_TINY = ((1, 1, 1), (1, 2, 5), (1, 3, 4), (1, 1, 4))  # maps inside one halo; the last two for the members that need W % 4 == 0
# (Cin, Cout) per what an id accepts.  40 = 2 * 16 + 8: the second 8-cout half of the last tile is masked out entirely (coA + 8 < Cout)
CONV_PAIRS = {"dma": ((32, 32), (32, 24)), "ks": ((64, 64), (64, 40)), "split": ((64, 64), (64, 40)), "fp32": ((39, 39), (7, 40)),
              "s2": ((39, 40), (7, 24))}
CONV_GUARD = 4096
CONV_SENTINEL = 1.2345e-3
CONV_REFUSED = []  # (cfg, what) of the documented refusals met by the last checks run: for the report
_CONV_REFS = {}    # case key -> the inputs, fp64 / fp32 references and tolerance terms: once per process, never written to
_CONV_DEV = {}     # (case key, device) -> the inputs on the device


def conv_lib():
    """the library's host-side table functions (family, stride, packed size per id): they need no device"""
    from drba_amd import _lib
    return _lib.load()


def conv_id_class(lib, cfg):
    """which layers an id accepts, asked of the library as check_conv_layers does: "s2" (a stride-2 tile), "fp32" (family 0), "dma"
    (family 2 and its family-4 member: Cin = 32, Cout <= 32), "ks" (family 3 and its member: Cin = 64 .. 192), "split" (the rest)"""
    fam = lib.drba_conv3x3_cfg_family(cfg)
    pf = lambda ci, co: lib.drba_conv3x3_packed_floats(ci, co, cfg)  # noqa: E731
    if lib.drba_conv3x3_cfg_stride(cfg) == 2:
        return "s2"
    if fam == 0:
        return "fp32"
    if fam == 2 or (fam == 4 and pf(32, 40) == 0 and pf(32, 32) > 0):
        return "dma"
    if fam == 3 or (fam == 4 and pf(32, 32) == 0):
        return "ks"
    return "split"


def conv_form_pairs(form, cls):
    pairs = CONV_PAIRS[cls]
    if form.cout is not None:
        return ((pairs[0][0], form.cout),)
    if form.res in ("in", "same", "copy"):  # the residual is the input: Cin == Cout
        return tuple(p for p in pairs if p[0] == p[1])[:1]
    return pairs


def conv_form_ref(form, x, wt, b, beta, res, res2, stride, dtype):
    """include/drba_hip.h:432-438 in `dtype`: PReLU(pre_slope) on the input, the convolution, y = acc + bias, then y * beta[c] +
    residual or y + residual (+ residual2), then the activation.  -> (output, y before the activation)"""
    c = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    xin = c(x)
    if form.pre_slope is not None:
        xin = torch.where(xin > 0, xin, xin * form.pre_slope)
    y = F.conv2d(xin, c(wt), c(b), stride=stride, padding=1)
    r = c(x) if form.res in ("in", "same", "copy") else c(res)  # (the residual is the input as it is, not its pre-activation)
    if beta is not None:
        y = y * c(beta).view(1, -1, 1, 1) + r
    else:
        if r is not None:
            y = y + r
        if res2 is not None:
            y = y + c(res2)
    if form.act in (True, "lrelu"):
        out = torch.where(y > 0, y, y * 0.2)
    elif form.act == "prelu":
        out = torch.where(y > 0, y, y * form.post_slope)
    elif form.act == "relu":
        out = torch.relu(y)
    elif form.act == "tanh10":
        out = torch.tanh(y) * 10.0
    else:
        out = y
    return out, y


def _finite_max(t):
    fin = t[torch.isfinite(t)]
    return float(fin.abs().max()) if fin.numel() else 0.0


def conv_case(form, cin, cout, stride, n, h, w, plant=False):
    """The inputs of one (form, channel pair, map) and their references, built at the first use and shared by every id.  The layer's
    weights depend on (form, cin, cout) only.  plant: one NaN in the input and -inf as the bias of one output channel; plant="input":
    the -inf is a second element of the input instead (its footprint's sums are -inf or +inf by the sign of the weight)."""
    key = (form.name, cin, cout, stride, n, h, w, plant)
    if key not in _CONV_REFS:
        k = CONV_FORMS.index(form)
        ws = 5000 + 97 * k + 13 * cin + cout                                  # the layer
        xs = 7000 + 97 * k + 13 * cin + cout + 1009 * h + 31 * w + n + stride  # its input on this map
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        # tanh * 10: inputs of unit scale, so that the outputs are not all saturated (asserted below)
        x = cases.rnd((n, cin, h, w), xs, 1.0 if form.act == "tanh10" else 2.0)
        wt = cases.rnd((cout, cin, 3, 3), ws, 1.0 / (cin * 9) ** 0.5)
        b = cases.rnd((cout,), ws + 1, 0.1) if form.bias else None
        beta = torch.rand(cout, generator=torch.Generator().manual_seed(ws + 2)) + 0.5 if form.beta else None
        res = cases.rnd((n, cout, ho, wo), xs + 1, 1.0) if form.res in ("other", "other2") else None
        res2 = cases.rnd((n, cout, ho, wo), xs + 2, 1.0) if form.res == "other2" else None
        if plant:
            x[0, min(1, cin - 1), h // 2, w // 3] = float("nan")
            if plant == "input":
                x[n - 1, 0, h - 1, w - 2] = float("-inf")
            else:
                b = b.clone()
                b[min(5, cout - 1)] = float("-inf")
        ref64, y64 = conv_form_ref(form, x, wt, b, beta, res, res2, stride, torch.float64)
        ref32, y32 = conv_form_ref(form, x, wt, b, beta, res, res2, stride, torch.float32)
        if form.act == "tanh10":  # the bar is set on y and multiplied by 10 (|tanh'| <= 1): a quarter of the |y| at least below 1
            assert float((y64.abs() < 1.0).double().mean()) >= 0.25, key
            a64, a32 = y64, y32
        else:
            a64, a32 = ref64, ref32
        if plant:
            assert bool(ref64.isnan().any()) and bool((y64 == float("-inf")).any()) and bool(torch.isfinite(ref64).any()), key
            assert plant != "input" or bool((ref64 == float("inf")).any()), key
        _CONV_REFS[key] = dict(x=x, wt=wt, b=b, beta=beta, res=res, res2=res2, ref64=ref64, refmax=_finite_max(a64), floor=_err(a32, a64),
                               out_shape=(n, cout, ho, wo))
    return _CONV_REFS[key]


def conv_tol(fam, form, case):
    """(tol, floor to carry in the row).  Families 1-4: 5e-6 max(1, |ref|max), the bar of check_conv_layers.  Family 0: rule_tol with
    the floor of the fp32 F.conv2d form of the same layer.  tanh * 10: the bar of y, times 10."""
    tol = rule_tol(case["refmax"], case["floor"]) if fam == 0 else 5e-6 * max(1.0, case["refmax"])
    if form.act == "tanh10":
        return 10.0 * tol, None
    return tol, (case["floor"] if fam == 0 else None)


def _conv_dev(key, case, dev):
    if (key, str(dev)) not in _CONV_DEV:
        _CONV_DEV[(key, str(dev))] = {k: None if case[k] is None else case[k].to(dev) for k in ("x", "res", "res2")}
    return _CONV_DEV[(key, str(dev))]


def conv_guarded(shape, dev):
    """-> (the allocation, `out`): `out` is a view of `shape`, prefilled with NaN, in the middle of one allocation that holds
    CONV_GUARD sentinel floats in front of it and behind it (the layout of test_softsplat_workspace_guard)"""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + 2 * CONV_GUARD,), CONV_SENTINEL, device=dev)
    buf[CONV_GUARD:CONV_GUARD + numel] = float("nan")
    return buf, buf[CONV_GUARD:CONV_GUARD + numel].view(shape)


def guard_row(op, name, buf, extra=""):
    numel = buf.numel() - 2 * CONV_GUARD
    return exact_row(op, f"{name}: the {CONV_GUARD} floats in front of and behind out", torch.cat([buf[:CONV_GUARD], buf[CONV_GUARD + numel:]]),
                     torch.full((2 * CONV_GUARD,), CONV_SENTINEL), extra)


def _refused(e):
    return type(e).__name__ == "DrbaHipError" and "(-2)" in str(e)  # DRBA_EUNSUPPORTED through _lib.check


def _tag(row, cfg, form, kind):
    row.cfg, row.form, row.kind = cfg, form, kind
    return row


def _conv_form_rows(rows, layers, ops, dev, lib, cfg, form, cin, cout, n, h, w, guard, plant=False):
    """the launch of one (id, form, channel pair, map): its value row, its guard row, or a failing row for anything but the one
    documented refusal (include/drba_hip.h: family 2 and its family-4 member need W % 4 == 0)"""
    op = "conv_forms"
    fam, stride, cls = lib.drba_conv3x3_cfg_family(cfg), lib.drba_conv3x3_cfg_stride(cfg), conv_id_class(lib, cfg)
    planted = " NaN, -inf in the input" if plant == "input" else " NaN, -inf" if plant else ""
    name = f"cfg{cfg} fam{fam} {form.name}{planted} [{n}x{cin}->{cout} {h}x{w} s{stride}]"
    try:
        case = conv_case(form, cin, cout, stride, n, h, w, plant)
        key = (form.name, cin, cout, stride, n, h, w, plant)
        d = _conv_dev(key, case, dev)
        if (form.name, cin, cout, cfg) not in layers:  # one layer per (form, channel pair, id): packed once, run on every map
            layers[(form.name, cin, cout, cfg)] = ops.Conv3x3(case["wt"], case["b"], stride, form.act, case["beta"], device=dev, cfg=cfg,
                                                              pre_slope=form.pre_slope, post_slope=form.post_slope)
        layer = layers[(form.name, cin, cout, cfg)]
        buf, out = conv_guarded(case["out_shape"], dev) if guard else (None, None)
        residual = d["x"] if form.res in ("in", "same") else d["x"].clone() if form.res == "copy" else d["res"]
        try:
            got = layer(d["x"], residual=residual, out=out, residual2=d["res2"])
        except Exception as e:  # noqa: BLE001
            if _refused(e) and cls == "dma" and w % 4 != 0:
                CONV_REFUSED.append((cfg, f"{n}x{h}x{w}"))
                return
            raise
        tol, floor = conv_tol(fam, form, case)
        if plant:
            assert floor is None or floor < float("inf"), name  # the fp32 form keeps the non-finite values where the reference has them
        extra = f"|ref|max={case['refmax']:.3g}" + ("" if fam else f" fp32_floor={case['floor']:.2e}")
        rows.append(_tag(Row(op, name, _err(got, case["ref64"]), tol, extra, floor, case["refmax"]), cfg, form.name, "nonfinite" if plant else "value"))
        if guard:
            rows.append(_tag(guard_row(op, name, buf), cfg, form.name, "guard"))
    except Exception as e:  # noqa: BLE001
        rows.append(_tag(Row(op, name, float("inf"), 0.0, f"EXC {type(e).__name__}: {e}"), cfg, form.name, "error"))


def check_conv_forms(dev, ops=None, cfgs=None, forms=None):
    """Every id (or `cfgs`) x every form (or the named `forms`) that applies to its stride x the channel pairs it accepts x CONV_MAPS
    (with out= guarded by sentinels) and, for the first pair, CONV_TINY."""
    ops = ops or default_ops()
    lib = conv_lib()
    rows, layers = [], {}
    del CONV_REFUSED[:]
    for cfg in range(lib.drba_conv3x3_num_cfgs()) if cfgs is None else cfgs:
        cls = conv_id_class(lib, cfg)
        for form in CONV_FORMS:
            if (forms is not None and form.name not in forms) or (cls == "s2" and form.res is not None):
                continue
            for k, (cin, cout) in enumerate(conv_form_pairs(form, cls)):
                if lib.drba_conv3x3_packed_floats(cin, cout, cfg) == 0:
                    continue
                for (n, h, w) in CONV_MAPS + (CONV_TINY if k == 0 else ()):
                    _conv_form_rows(rows, layers, ops, dev, lib, cfg, form, cin, cout, n, h, w, guard=(n, h, w) in CONV_MAPS)
    return rows


def conv_forms_missing(rows, lib, cfgs, forms=None):
    """(cfg, form) pairs that apply and have no accepted launch among `rows`: the completeness rule of the GPU tests"""
    have = {(r.cfg, r.form) for r in rows if getattr(r, "kind", None) == "value"}
    want = [(c, f.name) for c in cfgs for f in CONV_FORMS
            if (forms is None or f.name in forms) and not (conv_id_class(lib, c) == "s2" and f.res is not None)]
    return [p for p in want if p not in have]


def check_conv_relu_nonfinite(dev, ops=None, cfgs=None):
    """ReLU on a non-finite sum, per id and store path (W % 4 == 0 and != 0): torch.relu keeps a NaN and answers +0 for -inf.  The
    NaN is planted in the input (the sums of its 3 x 3 footprint are NaN in every output channel); the -inf is the bias of one
    output channel, so that the sum itself is -inf in every family -- a -inf activation is not representable in the split-operand
    loaders of families 1 - 4 (x - bf16(x) is NaN), which is the loader's matter and not the epilogue's.  Family 0 reads fp32
    operands as they are: its ids also take the row with both the NaN and the -inf in the input."""
    ops = ops or default_ops()
    lib = conv_lib()
    rows = []
    form = CONV_FORMS[1]
    assert form.act == "relu"
    for cfg in range(lib.drba_conv3x3_num_cfgs()) if cfgs is None else cfgs:
        cin, cout = conv_form_pairs(form, conv_id_class(lib, cfg))[0]
        if lib.drba_conv3x3_packed_floats(cin, cout, cfg) == 0:
            continue
        for (n, h, w) in CONV_MAPS:
            _conv_form_rows(rows, {}, ops, dev, lib, cfg, form, cin, cout, n, h, w, guard=False, plant=True)
            if lib.drba_conv3x3_cfg_family(cfg) == 0:
                _conv_form_rows(rows, {}, ops, dev, lib, cfg, form, cin, cout, n, h, w, guard=False, plant="input")
    # The family-4 kernels report every NaN they store into the device's sticky status word (ops.check_overflow raises on it at a
    # model's next step).  The NaN stored here is the one these rows ask for: the report is taken back once the kernels are done.
    clear = getattr(ops, "overflow_groups", None)
    if clear is not None:
        if torch.device(dev).type == "cuda":
            torch.cuda.synchronize(dev)
        clear(dev)
    return rows


DECONV_GUARD_CASES = ((1, 32, 52, 11, 45, True), (2, 32, 40, 9, 44, False))  # (N, Cin, Cout, H, W, pixel_shuffle)


def check_deconv_guard(dev, ops=None):
    """Deconv4x4 of every id, one map per pixel_shuffle value, into a guarded out=: the fp64 value row and the sentinels"""
    ops = ops or default_ops()
    lib = conv_lib()
    op, rows = "conv_forms", []
    for i, (n, cin, cout, h, w, ps) in enumerate(DECONV_GUARD_CASES):
        x = cases.rnd((n, cin, h, w), 9000 + i, 2.0)
        wt = cases.rnd((cin, cout, 4, 4), 9010 + i, 1.0 / (cin * 4) ** 0.5)
        b = cases.rnd((cout,), 9020 + i, 0.1)
        sh = lambda t: F.pixel_shuffle(t, 2) if ps else t  # noqa: E731
        ref64 = sh(F.conv_transpose2d(x.double(), wt.double(), b.double(), stride=2, padding=1))
        ref32 = sh(F.conv_transpose2d(x, wt, b, stride=2, padding=1))
        refmax, floor = _finite_max(ref64), _err(ref32, ref64)
        xd = x.to(dev)
        for cfg in range(lib.drba_deconv4x4_num_cfgs()):
            fam = lib.drba_deconv4x4_cfg_family(cfg)
            name = f"deconv cfg{cfg} fam{fam} [{n}x{cin}->{cout} {h}x{w} ps={int(ps)}]"
            if lib.drba_deconv4x4_packed_floats(cin, cout, cfg) == 0:
                continue
            try:
                buf, out = conv_guarded(tuple(ref64.shape), dev)
                got = ops.Deconv4x4(wt, b, ps, device=dev, cfg=cfg)(xd, out=out)
                tol = rule_tol(refmax, floor) if fam == 0 else 5e-6 * max(1.0, refmax)
                rows.append(_tag(Row(op, name, _err(got, ref64), tol, f"|ref|max={refmax:.3g}", floor if fam == 0 else None, refmax), cfg, "deconv", "value"))
                rows.append(_tag(guard_row(op, name, buf), cfg, "deconv", "guard"))
            except Exception as e:  # noqa: BLE001
                rows.append(_tag(Row(op, name, float("inf"), 0.0, f"EXC {type(e).__name__}: {e}"), cfg, "deconv", "error"))
    return rows


SHUFFLE_GUARD_CASES = ((2, 32, 72, 9, 68), (1, 64, 64, 11, 44))  # (N, Cin, Cout, H, W): W % 4 == 0, Cout % 4 == 0, ragged tiles


def shuffle_launch(ops, layer, xd, out, cfg):
    """drba_conv3x3_shuffle of `layer` with a pinned id storing to `out`, as check_conv_layers issues it; -> its return code
    (a stand-in namespace brings its own conv3x3_shuffle_launch)"""
    own = getattr(ops, "conv3x3_shuffle_launch", None)
    if own is not None:
        return own(layer, xd, out, cfg)
    import ctypes as C
    n, cin, h, w = xd.shape
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    return ops._lib.load().drba_conv3x3_shuffle(p(xd), p(layer._pack(cfg)), p(layer.bias), p(out), n, cin, h, w, layer.cout, layer.act,
                                               layer.post_slope, cfg, ops._stream())


def check_shuffle_guard(dev, ops=None):
    """conv3x3 + PixelShuffle(2) in the store with act="prelu" (the existing shuffle rows use act 0 and 1 only): every family-4
    stride-1 id that has the store form, pinned, into a guarded out; then the ops-level helper.  An id without the store form answers
    DRBA_EUNSUPPORTED (include/drba_hip.h, drba_conv3x3_shuffle); any other code is a failing row."""
    ops = ops or default_ops()
    lib = conv_lib()
    op, rows = "conv_forms", []
    for i, (n, cin, cout, h, w) in enumerate(SHUFFLE_GUARD_CASES):
        x = cases.rnd((n, cin, h, w), 9100 + i, 2.0)
        wt = cases.rnd((cout, cin, 3, 3), 9110 + i, 1.0 / (cin * 9) ** 0.5)
        b = cases.rnd((cout,), 9120 + i, 0.1)
        y = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
        ref64 = F.pixel_shuffle(torch.where(y > 0, y, y * 0.1), 2)
        refmax = _finite_max(ref64)
        tol = 5e-6 * max(1.0, refmax)  # family 4's bar
        layer = ops.Conv3x3(wt, b, 1, "prelu", None, device=dev, post_slope=0.1)
        xd = x.to(dev)
        accepted = 0
        for cfg in range(lib.drba_conv3x3_num_cfgs()):
            if lib.drba_conv3x3_cfg_family(cfg) != 4 or lib.drba_conv3x3_cfg_stride(cfg) != 1 or lib.drba_conv3x3_packed_floats(cin, cout, cfg) == 0:
                continue
            name = f"conv+shuffle prelu cfg{cfg} [{n}x{cin}->{cout} {h}x{w}]"
            try:
                buf, out = conv_guarded((n, cout // 4, 2 * h, 2 * w), dev)
                rc = shuffle_launch(ops, layer, xd, out, cfg)
                if rc == -2:
                    continue  # (DRBA_EUNSUPPORTED: the tile has no shuffle store form)
                if rc != 0:
                    raise RuntimeError(f"drba_conv3x3_shuffle returned {rc}")
                accepted += 1
                rows.append(_tag(Row(op, name, _err(out, ref64), tol, f"|ref|max={refmax:.3g}", None, refmax), cfg, "shuffle", "value"))
                rows.append(_tag(guard_row(op, name, buf), cfg, "shuffle", "guard"))
            except Exception as e:  # noqa: BLE001
                rows.append(_tag(Row(op, name, float("inf"), 0.0, f"EXC {type(e).__name__}: {e}"), cfg, "shuffle", "error"))
        rows.append(Row(op, f"conv+shuffle prelu [{n}x{cin}->{cout} {h}x{w}]: configurations that accept", 0.0 if accepted >= 2 else float("inf"), 1.0,
                        f"{accepted} ids"))
        rows.append(Row(op, f"ops.conv3x3_shuffle prelu [{n}x{cin}->{cout} {h}x{w}]", _err(ops.conv3x3_shuffle(layer, xd), ref64), tol,
                        f"|ref|max={refmax:.3g}", None, refmax))
    return rows


def check_conv_forms_all(dev, ops=None):
    """the family as the report prints it: forms x ids, ReLU on non-finite sums, the transposed convolution's and the shuffle store's guards"""
    return check_conv_forms(dev, ops) + check_conv_relu_nonfinite(dev, ops) + check_deconv_guard(dev, ops) + check_shuffle_guard(dev, ops)


# The persistent loops of conv_split.hip and conv_dma.hip (a workgroup takes tile after tile) in the two forms the 1080p rows of
# tests/test_gpu_fullsize.py do not cover: a batch of small maps, 32 -> 32, every stride-1 id that accepts the layer.
MANY_N = 128
MANY_MAP = (37, 76)
MANY_FORMS = ("resconv res is in", "pre+res+res2")
_MANY_DEV = {}


def conv_many_layer(ops, dev, form, cfg, n=MANY_N):
    """(layer, case) of a many-item row"""
    case = conv_case(form, 32, 32, 1, n, MANY_MAP[0], MANY_MAP[1])
    return ops.Conv3x3(case["wt"], case["b"], 1, form.act, case["beta"], device=dev, cfg=cfg, pre_slope=form.pre_slope, post_slope=form.post_slope), case


def conv_many_inputs(dev, form, n=MANY_N):
    """the case's inputs and its fp64 reference on the device (the error of 11.5 M elements is taken where they live)"""
    key = (form.name, n, str(dev))
    if key not in _MANY_DEV:
        case = conv_case(form, 32, 32, 1, n, MANY_MAP[0], MANY_MAP[1])
        _MANY_DEV[key] = {k: None if case[k] is None else case[k].to(dev) for k in ("x", "res", "res2", "ref64")}
    return _MANY_DEV[key]


def conv_many_ids(lib):
    return [c for c in range(lib.drba_conv3x3_num_cfgs()) if lib.drba_conv3x3_cfg_stride(c) == 1 and lib.drba_conv3x3_packed_floats(32, 32, c) > 0]


def check_conv_many(dev, ops=None, n=MANY_N, cfgs=None):
    ops = ops or default_ops()
    lib = conv_lib()
    op, rows = "conv_forms", []
    for form in (f for f in CONV_FORMS if f.name in MANY_FORMS):
        for cfg in conv_many_ids(lib) if cfgs is None else cfgs:
            fam = lib.drba_conv3x3_cfg_family(cfg)
            name = f"cfg{cfg} fam{fam} {form.name} [{n}x32->32 {MANY_MAP[0]}x{MANY_MAP[1]}]"
            try:
                layer, case = conv_many_layer(ops, dev, form, cfg, n)
                d = conv_many_inputs(dev, form, n)
                got = layer(d["x"], residual=d["x"] if form.res == "same" else d["res"], residual2=d["res2"])
                diff = (got.double() - d["ref64"]).abs().max()  # (all of the reference is finite: a NaN in `got` makes this NaN, a failing row)
                err = float(diff) if bool(torch.isfinite(diff)) else float("inf")
                tol, floor = conv_tol(fam, form, case)
                rows.append(_tag(Row(op, name, err, tol, f"|ref|max={case['refmax']:.3g}", floor, case["refmax"]), cfg, form.name, "value"))
            except Exception as e:  # noqa: BLE001
                rows.append(_tag(Row(op, name, float("inf"), 0.0, f"EXC {type(e).__name__}: {e}"), cfg, form.name, "error"))
    return rows


# ----------------------------------------------------------------------------------------- the GMFlow transformer kernels
# window_attn.hip, global_corr.hip, linear_split.hip at their dispatch edges.  The host rules that pick a form are restated here
# (as SCAN_PER_BLOCK is in test_gpu_op_parity.py) so that the row lists can be chosen -- and asserted -- to reach every form; the
# GPU tests read the form that actually ran from the kernel trace.
ATTN_KEYS = 64         # kKeys, drba_amd/csrc/window_attn.hip:42 and global_corr.hip:26: keys per chunk
ATTN_ROWS = 64         # kRows, window_attn.hip:41 and global_corr.hip:25: query rows per workgroup of the fp32 kernels
ATTN_TAB_CAP = 3968    # kTabCap, window_attn.hip:297: keys of one walk the two-term kernel's token table holds
LIN_WIDE_MIN = 1536    # wide_min, linear_split.hip:309: workgroups of 128 x 128 from which the two-term form takes 128-token tiles
GUARD = 4096           # sentinel floats behind an output / a workspace
SENTINEL = 1.2345e-3


def _cdiv(a, b):
    return -(-a // b)


def attn16_waves(L):
    """window_attn.hip:631-635"""
    return 8 if L >= 192 else 4


def attn_ksplit(nwin, L):
    """window_attn.hip:637-642: key runs of the fp32 kernel"""
    qtiles, chunks = _cdiv(L, ATTN_ROWS), _cdiv(L, ATTN_KEYS)
    if _cdiv(nwin, 8) * 8 * qtiles >= 2 * 256 or chunks < 8:
        return 1
    return 4 if chunks >= 16 else 2


def attn16_ksplit(nwin, L, waves):
    """window_attn.hip:647-660: key runs of the two-term kernel"""
    qtiles, chunks = _cdiv(L, 16 * waves), _cdiv(L, ATTN_KEYS)
    per_run, slots = _cdiv(nwin, 8) * 8 * qtiles, 256 * (1 if waves == 8 else 2)
    best, best_cost, ks = 1, -1, 1
    while ks <= 10 and (ks == 1 or chunks // ks >= 4):
        cost = _cdiv(per_run * ks, slots) * (2 * _cdiv(chunks, ks) + 5) + (3 if ks > 1 else 0)
        if best_cost < 0 or cost < best_cost:
            best, best_cost = ks, cost
        ks += 1
    return best


def gcorr_ksplit(L):
    """pick_ksplit, global_corr.hip:213-230"""
    qtiles, chunks = _cdiv(L, ATTN_ROWS), _cdiv(L, ATTN_KEYS)
    best, best_cost, ks = 1, 0x7fffffff, 1
    while ks <= 12 and chunks // ks >= 4:
        per_cu = _cdiv(qtiles * ks, 256)
        if per_cu > 3 and ks > 1:
            break
        cost = per_cu * (_cdiv(chunks, ks) + 2)
        if cost < best_cost:
            best, best_cost = ks, cost
        ks += 1
    return best


def attn_runs(c, terms):
    """key runs per window the default dispatch takes for case c (a workspace given)"""
    nwin, L = c.b * c.splits ** 2, (c.h // c.splits) * (c.w // c.splits)
    return attn16_ksplit(nwin, L, attn16_waves(L)) if terms == 2 else attn_ksplit(nwin, L)


def uneven(L, runs):
    """the last key run is shorter than the others (in chunks)"""
    return runs > 1 and _cdiv(L, ATTN_KEYS) % runs != 0


def two_term(x, shift=0):
    """x (fp32 values) as the two-term fp16 form holds it, in float64: h = fp16(x 2^-s), l = fp16((x 2^-s - h) 2048),
    x' = (h + l / 2048) 2^s (split2h, window_attn.hip:304-315; K with s = 4, :316)"""
    xs = x.double() * 2.0 ** -shift
    h = xs.to(torch.float16).double()
    lo = ((xs - h) * 2048.0).to(torch.float16).double()
    return (h + lo / 2048.0) * 2.0 ** shift


class AttnCase(collections.namedtuple("AttnCase", "name b h w splits shift amp scale seed kind")):
    @property
    def L(self):
        return (self.h // self.splits) * (self.w // self.splits)

    @property
    def nwin(self):
        return self.b * self.splits ** 2


S128 = 128 ** 0.5


def _ac(b, h, w, splits, shift, seed, amp=1.5, scale=S128, kind="plain", tag=""):
    wh, ww = h // splits, w // splits
    name = f"b{b} {h}x{w} splits{splits} shift{int(shift)} (L={wh * ww}={wh}x{ww}, {b * splits * splits} windows){tag}"
    return AttnCase(name, b, h, w, splits, shift, amp, scale, seed, kind)


ATTN_GEOMETRY = (
    # both sides of the 64-key chunk / the 64-row query tile: L = 63, 64, 65 from 7 x 9, 8 x 8, 5 x 13 (odd wh and ww with a shift:
    # sh = wh // 2 floors), with 4, 9 (splits 3) and 18 (b = 2, splits 3) windows
    _ac(1, 14, 18, 2, True, 5000), _ac(1, 24, 24, 3, True, 5001), _ac(2, 15, 39, 3, True, 5002), _ac(1, 7, 9, 1, False, 5003),
    # 127 (prime: one 1 x 127 window), 128 (8 x 16, 16 windows), 129 (3 x 43): the 128-row tile of the 8-wave form is not reached below 192
    _ac(1, 1, 127, 1, False, 5004), _ac(1, 32, 64, 4, True, 5005), _ac(1, 6, 86, 2, True, 5006),
    # the 4 / 8-wave switch at L = 192: 187 (11 x 17), 192 (12 x 16), 195 (13 x 15)
    _ac(1, 22, 34, 2, True, 5007), _ac(1, 24, 32, 2, True, 5008), _ac(1, 24, 32, 2, False, 5009), _ac(1, 13, 15, 1, False, 5010),
    # the two 128-row tiles of the 8-wave form: 255 (15 x 17), 256 (16 x 16), 257 (prime, 1 x 257)
    _ac(1, 30, 34, 2, True, 5011), _ac(1, 32, 32, 2, True, 5012), _ac(1, 1, 257, 1, False, 5013),
    # ww == 1 (the ww_magic special case, window_attn.hip:62, :685) on a window longer than one chunk: 70 x 1
    _ac(1, 140, 2, 2, False, 5014),
    # b = 2 with a shift on a shape whose default dispatch splits the keys (8 windows of 19 x 24 = 456: two runs in both kernels)
    _ac(2, 38, 48, 2, True, 5015),
)
ATTN_RUNS = (  # one window each; the smallest shapes that give 1..6 key runs (two-term) and 1, 2, 4 (fp32); see test_..._run_counts
    _ac(1, 13, 15, 1, False, 5020), _ac(1, 19, 24, 1, False, 5021), _ac(1, 18, 30, 1, False, 5022), _ac(1, 24, 30, 1, False, 5023),
    _ac(1, 28, 29, 1, False, 5024), _ac(1, 22, 44, 1, False, 5025), _ac(1, 33, 32, 1, False, 5026), _ac(1, 46, 46, 1, False, 5027),
    _ac(1, 58, 72, 1, False, 5028),
)
ATTN_PEAKED = (
    # the -100 mask decides: amplitude 3, scale 1 -- a masked key that scores 100 above the best unmasked one still takes the row
    _ac(1, 26, 30, 2, True, 5030, amp=3.0, scale=1.0, kind="mask", tag=" amp3 scale1"),
    _ac(1, 22, 34, 2, True, 5031, amp=3.0, scale=1.0, kind="mask", tag=" amp3 scale1"),
    # the running rescale: amplitude 6, the keys of the window in ascending order of their score for query rows 0..3
    _ac(1, 12, 25, 1, False, 5032, amp=6.0, kind="late", tag=" amp6 late maximum"),
)
ATTN_CASES = ATTN_GEOMETRY + ATTN_RUNS + ATTN_PEAKED
ATTN_TABLE = (  # through the C ABI with ws = NULL (one run walks every key), two-term: the table at its cap (62 chunks), and off
    _ac(1, 62, 64, 1, False, 5040), _ac(1, 63, 64, 1, False, 5041), _ac(1, 126, 128, 2, True, 5042))
ATTN_STRIDED = _ac(2, 14, 18, 2, True, 5050)
LATE_ROWS = 4
_MEMO = {}  # inputs and references per case: regenerated from seeds, computed once per process, never modified


def _late_order(q, k, v, scale):
    """keys (and their values) in ascending order of their score for query row 0; rows 1..3 are positive multiples of row 0"""
    for j in range(1, LATE_ROWS):
        q[:, j] = q[:, 0] * (1.0 + 0.25 * j)
    order = torch.argsort((k[0].double() @ q[0, 0].double()) / scale)
    return q, k[:, order].contiguous(), v[:, order].contiguous()


def attn_inputs(c):
    key = ("attn in", c)
    if key not in _MEMO:
        q, k, v = [cases.rnd((c.b, c.h * c.w, 128), c.seed * 3 + j, c.amp) for j in range(3)]
        if c.kind == "late":
            q, k, v = _late_order(q, k, v, c.scale)
        _MEMO[key] = (q, k, v)
    return _MEMO[key]


def attn_ref(q, k, v, c, masked=-100.0):
    """transformer.py:46-113 through the oracle, which divides by sqrt(C): a free scale goes into q"""
    wh, ww = c.h // c.splits, c.w // c.splits
    mask = None
    if c.shift:
        mask = ogm.shift_window_mask(c.h, c.w, wh, ww, wh // 2, ww // 2)
        if masked != -100.0:
            mask = mask.masked_fill(mask != 0, masked)
    return ogm.window_attention(q * (S128 / c.scale), k, v, c.splits, c.shift, c.h, c.w, mask)


def _attn_smax(q, k, c):
    """the largest |score| inside a window: what the fp32 evaluation's own error scales with"""
    def win(t):
        t = t.view(c.b, c.h, c.w, 128)
        if c.shift:
            t = torch.roll(t, shifts=(-((c.h // c.splits) // 2), -((c.w // c.splits) // 2)), dims=(1, 2))
        return ogm.split_feature(t, c.splits, channel_last=True).reshape(c.nwin, c.L, 128)
    return float(torch.matmul(win(q), win(k).transpose(1, 2)).abs().max()) / c.scale


def attn_refs(c):
    """{ref64, ref32, fmt_floor, smax, ...} of a case, with the conditions a peaked case exists for asserted before anything runs"""
    key = ("attn ref", c)
    if key in _MEMO:
        return _MEMO[key]
    q, k, v = attn_inputs(c)
    r = {"ref64": attn_ref(q.double(), k.double(), v.double(), c), "ref32": attn_ref(q, k, v, c), "smax": _attn_smax(q, k, c)}
    r["fmt_floor"] = _err(attn_ref(two_term(q), two_term(k, 4), two_term(v), c), r["ref64"])
    r["refmax"], r["floor"] = float(r["ref64"].abs().max()), _err(r["ref32"], r["ref64"])
    if c.kind == "mask":
        # decisive: with -inf for -100 the reference itself moves by >= 100 tolerances in >= 2 % of the output rows
        d = (attn_ref(q.double(), k.double(), v.double(), c, float("-inf")) - r["ref64"]).abs().amax(-1)
        tol = max(rule_tol(r["refmax"], r["floor"]), 3.0 * r["fmt_floor"])
        r["mask_diff"], r["mask_share"] = float(d.max()), float((d >= 100.0 * tol).float().mean())
        assert r["mask_share"] >= 0.02, (c.name, r["mask_diff"], r["mask_share"], tol)
    if c.kind == "late":
        s = (q[0, :LATE_ROWS].double() @ k[0].double().t()) / c.scale
        r["late_argmax"] = [int(i) for i in s.argmax(-1)]
        assert c.L > 4 * ATTN_KEYS and all(i // ATTN_KEYS == _cdiv(c.L, ATTN_KEYS) - 1 for i in r["late_argmax"]), r["late_argmax"]
        assert bool((s[:, ATTN_KEYS - 1::ATTN_KEYS].diff(dim=-1) > 1.0).all())  # the maximum moves by more than 1 at every chunk
    _MEMO[key] = r
    return r


def attn_row(op, c, terms, got, extra=""):
    """value row of a case: rule_tol; a two-term row: max(rule_tol, 3 x the format floor)"""
    r = attn_refs(c)
    tol = rule_tol(r["refmax"], r["floor"])
    if terms == 2:
        tol = max(tol, 3.0 * r["fmt_floor"])
    x = f"fp32_floor={r['floor']:.2e} fmt_floor={r['fmt_floor']:.2e} |ref|max={r['refmax']:.3g} |score|max={r['smax']:.3g}"
    if c.kind == "mask":
        x += f" -inf-mask moves the reference by {r['mask_diff']:.3g} in {100 * r['mask_share']:.1f} % of the rows"
    row = Row(op, f"terms={terms} {c.name}", _err(got, r["ref64"]), tol, f"{x} {extra}".rstrip(), r["floor"], r["refmax"])
    row.smax, row.fmt_floor, row.tol_rule, row.case, row.terms = r["smax"], r["fmt_floor"], "two-term" if terms == 2 else None, c, terms
    return row


def attn_layouts(q, k, v, dev):
    """name -> (q, k, v) on dev as the model's layers pass them: views with unequal row strides and column offsets"""
    b, n, _ = q.shape
    kv = torch.cat((k, v), -1).to(dev)                                   # cross attention: q alone, k | v one projection (ld 128 / 256 / 256)
    qkv = torch.cat((q, k, v), -1).to(dev)                               # self attention: one fused projection (ld 384)
    wide = torch.cat((torch.zeros(b, n, 64), q, torch.zeros(b, n, 8)), -1).to(dev)  # q at column 64 of a [.., 200] tensor, k and v alone
    return {"q contiguous, k | v of [.., 256]": (q.to(dev), kv[..., :128], kv[..., 128:]),
            "q | k | v of [.., 384]": (qkv[..., :128], qkv[..., 128:256], qkv[..., 256:]),
            "q at column 64 of [.., 200], k and v contiguous": (wide[..., 64:192], k.to(dev), v.to(dev))}


def _note_views(views, *ts):
    """the non-contiguous views a strided row hands to the operator (the GPU suite asserts that their addresses reach the C call)"""
    if views is not None:
        views.extend(t for t in ts if not t.is_contiguous())


def attn_strided_rows(dev, ops, views=None):
    """ATTN_STRIDED on views with unequal row strides, bit for bit against the same call on contiguous copies"""
    op, rows, c = "window_attention", [], ATTN_STRIDED
    q, k, v = attn_inputs(c)
    for terms in (3, 2):
        want = ops.window_attention(q.to(dev), k.to(dev), v.to(dev), c.h, c.w, c.splits, c.shift, c.scale, terms=terms)
        rows.append(attn_row(op, c, terms, want))
        for name, (qs, ks, vs) in attn_layouts(q, k, v, dev).items():
            assert not (qs.is_contiguous() and ks.is_contiguous() and vs.is_contiguous())
            _note_views(views, qs, ks, vs)
            got = ops.window_attention(qs, ks, vs, c.h, c.w, c.splits, c.shift, c.scale, terms=terms)
            rows.append(exact_row(op, f"terms={terms} b2 {name} == contiguous copies", got, want))
    return rows


def check_window_attention_edges(dev, ops=None):
    """ops.window_attention with 3 and 2 terms on every case of ATTN_CASES against fp64, and on strided views bit for bit against
    the same call on contiguous copies"""
    ops = ops or default_ops()
    op, rows = "window_attention", []
    for c in ATTN_CASES:
        attn_refs(c)  # (a peaked case asserts its condition here, before anything is launched)
        q, k, v = [t.to(dev) for t in attn_inputs(c)]
        for terms in (3, 2):
            got = ops.window_attention(q, k, v, c.h, c.w, c.splits, c.shift, c.scale, terms=terms)
            rows.append(attn_row(op, c, terms, got, f"runs={attn_runs(c, terms)}"))
    return rows + attn_strided_rows(dev, ops)


# ---- global_expect2
GCORR_MAPS = (  # (h, w): L = 63, 64, 65, 127, 128, 129; 1 x 70 and 70 x 1 (y = key / w with h = 1 and with w = 1); w > h and h > w
    (7, 9), (8, 8), (13, 5), (1, 127), (8, 16), (43, 3), (1, 70), (70, 1), (5, 31), (31, 5))
GCORR_RUNS = (  # ragged maps for 2..8 key runs; pick_ksplit first gives them at L = 449, 705, 961, 1217, 1473, 1729, 1985
    # one chunk past the first chunk count of 2, 3, 4 runs (9, 13, 17 chunks: uneven) and at the first chunk count of 5..8 (5..8 x 4 chunks)
    (19, 27), (21, 37), (27, 38), (24, 51), (37, 40), (29, 60), (35, 57),  # L = 513, 777, 1026, 1224, 1480, 1740, 1995
    (61, 21), (39, 46), (23, 89),  # L = 1281 (5 runs, the last of one chunk), 1794 (6, uneven), 2047 (8)
    # at the first chunk count of 2, 3, 4 runs: 8, 12, 16 chunks as even runs of the minimum of 4 chunks (chunks / ks >= 4)
    (19, 24), (24, 30), (22, 44))  # L = 456, 720, 968
GCORR_SEEDS = {m: 5100 + 3 * i for i, m in enumerate(GCORR_MAPS + GCORR_RUNS)}
GCORR_LATE = (12, 25)


def gcorr_inputs(h, w, seed, amp=0.9, late=False):
    key = ("gcorr in", h, w, seed, amp, late)
    if key not in _MEMO:
        L = h * w
        t0, t1, flow = cases.rnd((L, 128), seed, amp), cases.rnd((L, 128), seed + 1, amp), cases.rnd((2, L), seed + 2, 5.0)
        if late:
            q3, k3, f3 = _late_order(t0[None].clone(), t1[None], flow.t()[None].contiguous(), S128)
            t0, t1, flow = q3[0], k3[0], f3[0].t().contiguous()
        _MEMO[key] = (t0, t1, flow)
    return _MEMO[key]


def gcorr_ref(t0, t1, flow, h, w):
    """matching.py:7-38 through the oracle (features [1, C, h, w]) for the coordinate form; the same softmax applied to a flow
    (transformer.py:355-372) for the value form"""
    L = h * w
    f0, f1 = t0.t().reshape(1, 128, h, w), t1.t().reshape(1, 128, h, w)
    coords = ogm.global_correlation_softmax(f0, f1)[0].reshape(2, L)
    p = torch.softmax((t0 @ t1.t()) / S128, -1)
    return coords, (p @ flow.t()).t()


def gcorr_refs(h, w, seed, amp=0.9, late=False):
    key = ("gcorr ref", h, w, seed, amp, late)
    if key not in _MEMO:
        t0, t1, flow = gcorr_inputs(h, w, seed, amp, late)
        if late:
            s = (t0[:LATE_ROWS].double() @ t1.double().t()) / S128
            assert all(int(i) // ATTN_KEYS == _cdiv(h * w, ATTN_KEYS) - 1 for i in s.argmax(-1)), s.argmax(-1)
            assert bool((s[:, ATTN_KEYS - 1::ATTN_KEYS].diff(dim=-1) > 1.0).all())
        _MEMO[key] = gcorr_ref(t0.double(), t1.double(), flow.double(), h, w) + gcorr_ref(t0, t1, flow, h, w)
    return _MEMO[key]


def gcorr_rows(op, name, h, w, got_c, got_v, refs):
    """the coordinate row at the project's bar, max(2e-5, 3 floor) max(1, w / 16) (tests/gpu_checks.py check_global_expect2), and
    the value row at rule_tol"""
    c64, v64, c32, v32 = refs
    floor, refmax = _err(c32, c64), float(c64.abs().max())
    row = Row(op, f"coords {name}", _err(got_c, c64), max(2e-5, 3.0 * floor) * max(1.0, w / 16.0), f"fp32_floor={floor:.2e} |ref|max={refmax:.3g}",
              floor, refmax)
    row.tol_rule, row.w = "coords", w
    return [row, value_row(op, f"values {name}", got_v, v64, v32)]


def gcorr_strided_rows(dev, ops, views=None):
    """q contiguous with k a slice of a [L, 256] tensor, and the reverse: the same bits as on contiguous copies"""
    op, rows = "global_expect2", []
    h, w = GCORR_RUNS[0]
    t0, t1, flow = gcorr_inputs(h, w, GCORR_SEEDS[(h, w)])
    q, k, f = t0.to(dev), t1.to(dev), flow.to(dev)
    wide_k, wide_q = torch.cat((torch.zeros(h * w, 128), t1), 1).to(dev), torch.cat((t0, torch.zeros(h * w, 128)), 1).to(dev)
    _note_views(views, wide_k[:, 128:], wide_q[:, :128])
    for vals, what in ((None, "coords"), (f, "values")):
        want = ops.global_expect2(q, k, vals, w, S128)
        rows.append(exact_row(op, f"{what} {h}x{w} q contiguous, k = [:, 128:] of [L, 256] == contiguous copies",
                              ops.global_expect2(q, wide_k[:, 128:], vals, w, S128), want))
        rows.append(exact_row(op, f"{what} {h}x{w} q = [:, :128] of [L, 256], k contiguous == contiguous copies",
                              ops.global_expect2(wide_q[:, :128], k, vals, w, S128), want))
    return rows


def check_global_expect2_edges(dev, ops=None):
    ops = ops or default_ops()
    op, rows = "global_expect2", []

    def one(h, w, seed, tag="", **kw):
        t0, t1, flow = gcorr_inputs(h, w, seed, **kw)
        q, k = t0.to(dev), t1.to(dev)
        name = f"{h}x{w} (L={h * w}, runs={gcorr_ksplit(h * w)}){tag}"
        rows.extend(gcorr_rows(op, name, h, w, ops.global_expect2(q, k, None, w, S128), ops.global_expect2(q, k, flow.to(dev), w, S128),
                               gcorr_refs(h, w, seed, **kw)))

    for (h, w), seed in GCORR_SEEDS.items():
        one(h, w, seed)
    one(*GCORR_LATE, 5190, " amp3 late maximum", amp=3.0, late=True)
    return rows + gcorr_strided_rows(dev, ops)


# ---- linear_split
LIN_EDGES = (  # (M, K, N, bias, gelu): every M of (1, 15..17, 63..65, 127..129), every N of (1, 15..17, 40, 127..129, 384), every K
    (1, 32, 1, True, False), (15, 64, 15, False, True), (16, 128, 16, True, False), (17, 32, 17, False, False), (63, 64, 40, True, True),
    (64, 128, 127, False, False), (65, 32, 128, True, True), (127, 64, 129, True, False), (128, 128, 384, False, True),
    (129, 32, 129, False, True), (129, 128, 128, True, False), (65, 64, 129, True, True), (1, 128, 384, True, False))
LIN_CAT = ((32, 32), (32, 96), (96, 32), (128, 128))  # (K1, K2): the split at the first chunk, at the last, and in the middle
LIN_WIDE = ((6100, True), (6016, False))              # (M, the 128-token form runs) at K = 32, N = 4096, two terms
LIN_WIDE_KN = (32, 4096)
LIN_LN = ((70, 64), (129, 128), (1, 32))              # (M, K) of the LayerNorm rows: ragged against the 64-token tile
LIN_LN_ILL_MIN_M = 64  # the ill-conditioned row's bar is 3 x a measured floor: not taken from a single row of 128 values
LIN_TERMS = (3, 2)


def lin_row(op, name, got, ref64, ref32, bar):
    """the bar the project holds linear_split to (tests/gpu_checks.py check_linear_split): 5e-6 max(1, |ref|max) for the GEMM forms,
    1e-5 max(1, |ref|max) with the LayerNorm epilogue; the fp32 torch floor is printed, it sets nothing"""
    floor, refmax = _err(ref32, ref64), float(ref64.abs().max())
    row = Row(op, name, _err(got, ref64), bar * max(1.0, refmax), f"fp32_floor={floor:.2e} |ref|max={refmax:.3g}", floor, refmax)
    row.tol_rule, row.bar = "linear", bar
    return row


def _lin_ref(x, w, b, gelu=False):
    y = F.linear(x, w, b)
    return F.gelu(y) if gelu else y


def _ln_ref(x, w, b, lw, lb, res):
    y = F.layer_norm(F.linear(x, w, b), (128,), lw, lb, 1e-5)
    return y if res is None else res + y


def _dbl(*ts):
    return [None if t is None else t.double() for t in ts]


def _sliced(x, pad_front, pad_back, dev):
    """x [M, K] as columns [pad_front : pad_front + K] of a wider tensor on dev (row stride and offset multiples of 4 floats)"""
    m, k = x.shape
    wide = torch.cat((torch.full((m, pad_front), 7.0), x, torch.full((m, pad_back), -7.0)), 1).to(dev)
    return wide[:, pad_front:pad_front + k]


def lin_ln_cases():
    """name -> (x, w, b, ln_w, ln_b, residual, ill): the LayerNorm epilogue's designed rows"""
    key = "lin ln"
    if key in _MEMO:
        return _MEMO[key]
    out = {}
    for i, (m, k) in enumerate(LIN_LN):
        s = 5400 + 10 * i
        x, w = cases.rnd((m, k), s, 2.0), cases.rnd((128, k), s + 1, 1.0 / k ** 0.5)
        lw, lb, res = cases.rnd((128,), s + 2, 0.3) + 1.0, cases.rnd((128,), s + 3, 0.1), cases.rnd((m, 128), s + 4, 1.0)
        b = cases.rnd((128,), s + 5, 0.1)
        out[f"[{m}x{k}] bias=1 residual=1"] = (x, w, b, lw, lb, res, False)
        out[f"[{m}x{k}] bias=0 residual=0"] = (x, w, None, lw, lb, None, False)
        # rows whose 128 pre-norm outputs are all equal (zero input rows): variance 0, eps decides, the answer is ln_b (+ residual).
        # The constant is 0.75: every partial sum of equal 0.75s is exact in fp32 in any order, so the mean is exact and no fp32
        # evaluation is excused by its own rounding (with 0.7 a sum's last-bit error, times 1 / sqrt(eps) = 316, is 1e-4)
        xz = x.clone()
        xz[[0, m // 2, m - 1]] = 0.0
        out[f"[{m}x{k}] zero rows, bias = 0.75: variance 0, residual=1"] = (xz, w, torch.full((128,), 0.75), lw, lb, res, False)
        out[f"[{m}x{k}] zero rows, no bias: variance 0, residual=0"] = (xz, w, None, lw, lb, None, False)
        # mean ~ 100, deviation ~ 0.1: a one-pass variance (E x^2 - mean^2) has nothing left of 0.01 next to 1e4 in fp32
        bm = 100.0 + cases.rnd((128,), s + 6, 0.1)
        if m >= LIN_LN_ILL_MIN_M:
            out[f"[{m}x{k}] mean 100 deviation 0.1 residual=1"] = (x * 0.02, w, bm, lw, lb, res, True)
    _MEMO[key] = out
    return out


def lin_gelu_case():
    """pre-activations placed exactly: w[n, n % 32] = 1, so y[m, n] = x[m, n % 32]: [-12, 12], 0 and -0, the erf's saturation"""
    x = torch.linspace(-12.0, 12.0, 65 * 32).view(65, 32).clone()
    x[3, :4] = torch.tensor([0.0, -0.0, 12.0, -12.0])
    x[64, 28:] = torch.tensor([-5.5, 5.5, -8.0, 8.0])
    w = torch.zeros(64, 32)
    w[torch.arange(64), torch.arange(64) % 32] = 1.0
    return x, w


def lin_cat_rows(dev, ops, views=None):
    """cat(x1, x2) read in place, x1 and x2 views with different row strides and column offsets"""
    op, rows = "linear_split", []
    D = lambda t: None if t is None else t.to(dev)  # noqa: E731
    for i, (k1, k2) in enumerate(LIN_CAT):
        m, n, gelu = 70, 129, bool(i % 2)
        x1, x2, w = cases.rnd((m, k1), 5300 + 4 * i, 2.0), cases.rnd((m, k2), 5301 + 4 * i, 2.0), cases.rnd((n, k1 + k2), 5302 + 4 * i, 1.0 / (k1 + k2) ** 0.5)
        b = cases.rnd((n,), 5303 + 4 * i, 0.5)
        xc = torch.cat((x1, x2), 1)
        ref64, ref32 = _lin_ref(*_dbl(xc, w, b), gelu), _lin_ref(xc, w, b, gelu)
        for terms in LIN_TERMS:
            layer = ops.LinearSplit(w, b, gelu=gelu, device=dev, terms=terms)
            v1, v2 = _sliced(x1, 8, 16, dev), _sliced(x2, 4, 4, dev)
            assert v1.stride(0) != v2.stride(0) and not v1.is_contiguous() and not v2.is_contiguous()
            _note_views(views, v1, v2)
            got = layer.cat(v1, v2)
            name = f"terms={terms} cat K1={k1} K2={k2} [{m}] -> {n} gelu={int(gelu)} strided views"
            rows.append(lin_row(op, name, got, ref64, ref32, 5e-6))
            rows.append(exact_row(op, f"{name} == the concatenated contiguous tensor", got, layer(D(xc))))
    return rows


def check_linear_split_edges(dev, ops=None):
    ops = ops or default_ops()
    op, rows = "linear_split", []
    D = lambda t: None if t is None else t.to(dev)  # noqa: E731
    for i, (m, k, n, bias, gelu) in enumerate(LIN_EDGES):
        x, w = cases.rnd((m, k), 5200 + 3 * i, 2.0), cases.rnd((n, k), 5201 + 3 * i, 1.0 / k ** 0.5)
        b = cases.rnd((n,), 5202 + 3 * i, 0.5) if bias else None
        ref64, ref32 = _lin_ref(*_dbl(x, w, b), gelu), _lin_ref(x, w, b, gelu)
        for terms in LIN_TERMS:
            got = ops.LinearSplit(w, b, gelu=gelu, device=dev, terms=terms)(D(x))
            rows.append(lin_row(op, f"terms={terms} [{m}x{k}] -> {n} gelu={int(gelu)} bias={int(bias)}", got, ref64, ref32, 5e-6))
    rows += lin_cat_rows(dev, ops)
    # the 128-token form of the two-term kernel and the last shape below it
    k, n = LIN_WIDE_KN
    xw, ww = cases.rnd((LIN_WIDE[0][0], k), 5350, 2.0), cases.rnd((n, k), 5351, 1.0 / k ** 0.5)
    for gelu in (False, True):
        r64, r32 = _lin_ref(xw.double(), ww.double(), None, gelu), _lin_ref(xw, ww, None, gelu)
        layer = ops.LinearSplit(ww, None, gelu=gelu, device=dev, terms=2)
        for m, wide in LIN_WIDE:
            rows.append(lin_row(op, f"terms=2 [{m}x{k}] -> {n} gelu={int(gelu)} {'128' if wide else '64'}-token tiles", layer(D(xw[:m])), r64[:m], r32[:m], 5e-6))
        del r64, r32
    # GELU over [-12, 12]: 1 - erf underflows, x * (1 + erf) cancels: the fp32 formula's own error sets the bar
    x, w = lin_gelu_case()
    for terms in LIN_TERMS:
        got = ops.LinearSplit(w, None, gelu=True, device=dev, terms=terms)(D(x))
        ref64 = _lin_ref(x.double(), w.double(), None, True)
        rows.append(value_row(op, f"terms={terms} GELU pre-activations in [-12, 12], 0 and -0", got, ref64, _lin_ref(x, w, None, True)))
        # the sign of zero, which a difference cannot see: inputs 0 and -0 (features 0, 1 and 32, 33 of token 3) give the pre-activation
        # +0 -- the sum also holds the +0 products of the other input zero -- and GELU(+0) is +0, not -0
        zeros = ref64[3, [0, 1, 32, 33]].float()
        assert _mismatches(zeros, torch.zeros(4)) == 0
        rows.append(exact_row(op, f"terms={terms} GELU of the pre-activations from inputs 0 and -0 is +0", got[3, [0, 1, 32, 33]], zeros))
    # LayerNorm epilogue
    for name, (x, w, b, lw, lb, res, ill) in lin_ln_cases().items():
        ref64, ref32 = _ln_ref(*_dbl(x, w, b, lw, lb, res)), _ln_ref(x, w, b, lw, lb, res)
        for terms in LIN_TERMS:
            got = ops.LinearSplit(w, b, device=dev, terms=terms).layernorm(D(x), D(lw), D(lb), D(res))
            full = f"terms={terms} + LayerNorm {name}"
            rows.append(value_row(op, full, got, ref64, ref32) if ill else lin_row(op, full, got, ref64, ref32, 1e-5))
    return rows


# ----------------------------------------------------------------------------------------- the fused IFNet encoder
# head_fused.hip (exact-fp32 MFMA) and head_fused16.hip (two fp16 terms per operand; what the pipeline runs): Head (IFNet_HDv3.py:23-47)
# as one kernel.  A workgroup owns a 16 x 64 output tile = 8 x 32 half-resolution positions and computes a 14 x 38 region (row
# stride 40) of cnn0 around it; the tile geometry is restated here so that the shapes can be chosen -- and asserted -- to reach every
# edge of it.  The GPU tests read the kernel that ran and its grid from the trace.
HEAD_H2, HEAD_W2 = 8, 32    # H2, W2, head_fused.hip:37 / head_fused16.hip:37: half-resolution positions per workgroup
HEAD_RR, HEAD_RS = 14, 40   # RR, RS, head_fused.hip:38-39: region rows, region row stride (what the `interior` test of :98 uses)
HEAD_ACT_SHIFT = 4          # kSplitActShift: the two-term form holds an activation as two fp16 terms of x / 16
HEAD_EDGES = ("one tile", "W%8==4", "ring", "interior", "tiles_x>8", "tiles_y>8")


def head_tiles(h, w):
    """(tiles_x, tiles_y) of the launch"""
    return _cdiv(w // 2, HEAD_W2), _cdiv(h // 2, HEAD_H2)


def head_edges(h, w):
    """which edges of the tile geometry an H x W frame reaches, from H, W and the constants above"""
    hh, wh = h // 2, w // 2
    nx, ny = head_tiles(h, w)
    rows_in = any(HEAD_H2 * ty - 3 >= 0 and HEAD_H2 * ty - 3 + HEAD_RR <= hh for ty in range(ny))   # rm >= 0 && rm + RR <= Hh
    cols_in = any(HEAD_W2 * tx - 3 >= 0 and HEAD_W2 * tx - 3 + HEAD_RS <= wh for tx in range(nx))   # rn >= 0 && rn + RS <= Wh
    is_ = {"one tile": nx == 1 and ny == 1, "W%8==4": w % 8 == 4, "interior": rows_in and cols_in, "tiles_x>8": nx > 8, "tiles_y>8": ny > 8,
           "ring": (nx, ny) == (2, 2) and hh - HEAD_H2 == 3 and wh - HEAD_W2 == 6}  # the second tiles hold exactly the three rings
    return frozenset(k for k, v in is_.items() if v)


HEAD_CASES = (  # (H, W, the edges it reaches): the smallest frame of each
    (2, 4, ("one tile", "W%8==4")),      # the smallest accepted frame (Hh 1, Wh 2): every position of every layer is border
    (6, 12, ("one tile", "W%8==4")),     # odd Hh
    (16, 64, ("one tile",)),             # exactly one full tile
    (18, 68, ("W%8==4",)),               # one row / two columns into a second tile each way
    (22, 76, ("ring", "W%8==4")),
    (38, 140, ("interior", "W%8==4")),   # 3 x 3 tiles, tile (1, 1): rm + 14 = 19 <= 19, rn + 40 = 69 <= 70
    (40, 144, ("interior",)),
    (16, 516, ("tiles_x>8", "W%8==4")),  # 1 x 9 tiles: a full strip of 8 and the narrow last strip
    (130, 4, ("tiles_y>8", "W%8==4")))   # 9 x 1 tiles: two tile rows per band, the last band short
for _h, _w, _e in HEAD_CASES:
    assert _h % 2 == 0 and _w % 4 == 0 and head_edges(_h, _w) == frozenset(_e), (_h, _w, sorted(head_edges(_h, _w)))
assert frozenset().union(*(c[2] for c in HEAD_CASES)) == frozenset(HEAD_EDGES)
assert (16, 64) in [c[:2] for c in HEAD_CASES] and head_tiles(18, 68) == (2, 2) and head_tiles(38, 140) == (3, 3)
HEAD_EXTRA = ((18, 68), (38, 140))          # the shapes that also take the frames that are not rand
HEAD_NAN = (38, 140, 1, 15, 63)             # (H, W, channel, y, x) of the NaN pixel: the seam of tiles (0, 0), (1, 0), (0, 1), (1, 1)
HEAD_NAN_CONE = ((9, 22), (57, 70))         # rows, columns (inclusive) of all 16 channels it reaches: 7 pixels each way, from (14, 62) / (15, 63)
HEAD_REFUSED = ((2, 16, 24), (1, 17, 36), (1, 18, 70))  # (N, H, W) ops.head_fused does not take: a batch, odd H, W % 4 == 2
HEAD_BATCH = (3, 18, 68)                    # (N, H, W) of the C-ABI rows of the GPU suite


def head_weights(kind):
    """[w0, b0, w1, b1, w2, b2, w3, b3] (fp32): "synth": encode.* of synth.ifnet_state_dict(seed=0) (biases of 0.02); "unit bias": a
    seeded set with fan-in scaled weights and N(0, 1) biases -- a ring that is not zeroed holds lrelu(bias) and the like, loud in every layer"""
    key = ("head w", kind)
    if key not in _MEMO:
        if kind == "synth":
            sd = synth.ifnet_state_dict(seed=0)
            _MEMO[key] = [sd[f"encode.cnn{k}.{p}"] for k in range(4) for p in ("weight", "bias")]
        else:
            shapes = ((16, 3, 3, 3), (16, 16, 3, 3), (16, 16, 3, 3), (16, 16, 4, 4))
            fan = (27, 144, 144, 64)
            _MEMO[key] = [t for k in range(4) for t in (cases.rnd(shapes[k], 6100 + 2 * k, 1.0 / fan[k] ** 0.5), cases.rnd((16,), 6101 + 2 * k, 1.0))]
    return _MEMO[key]


def head_ref(x, wts, dtype=torch.float64, fmt=False):
    """Head (IFNet_HDv3.py:23-47) in `dtype`.  fmt: the float64 layers on what the two-term form can hold -- weights as two fp16 terms,
    the frame and every intermediate as two fp16 terms of x / 16 (split again at every layer, as the kernel writes its LDS planes)"""
    wt = (lambda t: two_term(t)) if fmt else (lambda t: t.to(dtype))          # noqa: E731
    act = (lambda t: two_term(t, HEAD_ACT_SHIFT)) if fmt else (lambda t: t)   # noqa: E731
    w0, b0, w1, b1, w2, b2, w3, b3 = wts
    y = F.leaky_relu(F.conv2d(act(x.to(dtype)), wt(w0), b0.to(dtype), stride=2, padding=1), 0.2)
    y = F.leaky_relu(F.conv2d(act(y), wt(w1), b1.to(dtype), padding=1), 0.2)
    y = F.leaky_relu(F.conv2d(act(y), wt(w2), b2.to(dtype), padding=1), 0.2)
    return F.conv_transpose2d(act(y), wt(w3), b3.to(dtype), stride=2, padding=1)


def head_frame(h, w, kind, n=1):
    """the frame [n, 3, h, w] of an input kind, from a seed of (h, w, kind)"""
    seed = 6200 + 7 * h + w + 1000 * HEAD_KINDS.index("rand" if kind == "NaN pixel" else kind)  # (the NaN goes into the rand frame)
    if kind == "zero frame":
        return torch.zeros(n, 3, h, w)
    if kind in ("rand", "NaN pixel"):
        x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))
        if kind == "NaN pixel":
            assert (h, w) == HEAD_NAN[:2]
            x[0, HEAD_NAN[2], HEAD_NAN[3], HEAD_NAN[4]] = float("nan")
        return x
    return cases.rnd((n, 3, h, w), seed, {"randn*1e3": 1e3, "randn*1e-3": 1e-3}[kind])


HEAD_KINDS = ("rand", "zero frame", "randn*1e3", "randn*1e-3", "NaN pixel")
HEAD_WEIGHTS = {"zero frame": "unit bias"}  # input kind -> weight set (default "synth")


def head_inputs():
    """[(H, W, input kind, the forms it runs in: two-term False / True)]"""
    out = [(h, w, "rand", (False, True)) for h, w, _ in HEAD_CASES]
    for h, w in HEAD_EXTRA:
        out += [(h, w, kind, (False, True)) for kind in HEAD_KINDS[1:4]]
    return out + [HEAD_NAN[:2] + ("NaN pixel", (False,))]  # (the two-term form reports a NaN it stores: the GPU suite's own test)


def head_refs(h, w, kind, n=1):
    """{x, wkind, ref64, ref32, fmt_floor} of an input: computed once per process, never written to"""
    key = ("head ref", h, w, kind, n)
    if key not in _MEMO:
        x, wkind = head_frame(h, w, kind, n), HEAD_WEIGHTS.get(kind, "synth")
        wts = head_weights(wkind)
        r = {"x": x, "wkind": wkind, "ref64": head_ref(x, wts), "ref32": head_ref(x, wts, torch.float32)}
        r["fmt_floor"] = _err(head_ref(x, wts, fmt=True), r["ref64"])
        _MEMO[key] = r
    return _MEMO[key]


def head_layers(ops, dev, wkind):
    """((cnn0, cnn1, cnn2, cnn3), holder) as ops.head_fused takes them, built from the namespace's own layer classes"""
    import types
    w0, b0, w1, b1, w2, b2, w3, b3 = head_weights(wkind)
    return (ops.Conv3x3(w0, b0, stride=2, act=True, device=dev), ops.Conv3x3(w1, b1, stride=1, act=True, device=dev),
            ops.Conv3x3(w2, b2, stride=1, act=True, device=dev), ops.Deconv4x4(w3, b3, pixel_shuffle=False, device=dev)), types.SimpleNamespace()


def pair_layout(f):
    """[1, 16, H, W] -> [8, H, W, 2] by torch indexing (as check_layouts states pair_interleaved)"""
    _, c, h, w = f.shape
    return f.detach().cpu()[0].view(c // 2, 2, h, w).permute(0, 2, 3, 1).contiguous()


def head_value_row(op, name, got, r, two, extra=""):
    """the planar result against fp64 under the series' one rule; a two-term row also carries and prints the format floor (no bar of
    its own: tests/test_op_checks_cpu.py asserts that 3 x fmt_floor stays below the rule's tolerance on every row)"""
    row = value_row(op, name, got, r["ref64"], r["ref32"], (f"fmt_floor={r['fmt_floor']:.2e} " if two else "") + extra)
    row.two, row.fmt_floor = two, r["fmt_floor"]
    return row


def check_head_fused(dev, ops=None):
    """ops.head_fused in both forms (HEAD_TWO_TERM False: head_fused.hip, True: head_fused16.hip) on every shape of HEAD_CASES with
    uniform [0, 1) frames, and at HEAD_EXTRA on an all-zero frame (unit-bias weights), on signed frames of scale 1e3 and 1e-3 and, fp32
    form, with one NaN pixel at a seam of four tiles.  Per (input, form): the planar result against the four fp64 layers; the pair
    copy attached to it, the planar=False result and features_planar of that, each bit for bit against the layout they restate; the
    pair-only tag.  Then the shapes ops.head_fused does not take (None).  There is no inf input: both kernels pad K with zero-weight
    taps that read a tap of the same position again, so 0 * inf gives NaN where the reference keeps inf, and inf is outside the
    documented input range of both forms."""
    ops = ops or default_ops()
    op, rows, inf = "head_fused", [], float("inf")
    try:
        for two in (False, True):
            ops.HEAD_TWO_TERM = two
            form = "two-term" if two else "fp32"
            built = {k: head_layers(ops, dev, k) for k in ("synth", "unit bias")}
            for h, w, kind, forms in head_inputs():
                if two not in forms:
                    continue
                name = f"{form} {kind} {h}x{w}"
                try:
                    r = head_refs(h, w, kind)
                    layers, holder = built[r["wkind"]]
                    x = r["x"].to(dev)
                    f = ops.head_fused(x, layers, holder)
                    fp = getattr(f, "_drba_pair", None)
                    if f is None or fp is None:
                        rows.append(Row(op, f"{name}: planar", inf, 0.0, "not taken" if f is None else "no _drba_pair copy on the result"))
                        continue
                    nx, ny = head_tiles(h, w)
                    rows.append(head_value_row(op, f"{name}: planar vs fp64", f, r, two, f"tiles={nx}x{ny}"))
                    rows.append(exact_row(op, f"{name}: pair copy == the pair layout of the planar result", fp, pair_layout(f)))
                    f2 = ops.head_fused(x, layers, holder, planar=False)
                    rows.append(exact_row(op, f"{name}: planar=False == the pair copy of the planar call", f2, fp))
                    tagged = bool(getattr(f2, "_drba_is_pair", False)) and bool(ops.is_pair(f2))  # (at H = 2 the shape alone does not say so)
                    rows.append(Row(op, f"{name}: planar=False result carries the pair tag", 0.0 if tagged else inf, 0.0, f"shape {tuple(f2.shape)}"))
                    rows.append(exact_row(op, f"{name}: features_planar(planar=False) == planar", ops.features_planar(f2), f))
                except Exception as e:  # noqa: BLE001
                    rows.append(Row(op, name, inf, 0.0, f"EXC {type(e).__name__}: {e}"))
            layers, holder = built["synth"]
            for n, h, w in HEAD_REFUSED:
                got = ops.head_fused(head_frame(h, w, "rand", n).to(dev), layers, holder)
                rows.append(Row(op, f"{form} [{n}, 3, {h}, {w}] is not taken", 0.0 if got is None else inf, 0.0, "None: the caller runs the layers"))
    finally:
        ops.HEAD_FUSED, ops.HEAD_TWO_TERM = True, None
    return rows


# ----------------------------------------------------------------------------------------- the fused RIFE splats
# splat_long_prepass / splat_tiled (and the _det pair) of splat_warp.hip: all of drba_flow_reverse, drba_drm_rife_linear(_batch) and
# drba_drm_rife_nonlinear(_batch), against rife.py:59-73 and drm.py:65-107 as oracle/ops.py and oracle/drm.py restate them:
#   flow reversal        -2 * avg-splat(flow, flow), holes 2 * max(H, W);
#   linear / non-linear  avg-splat(u, self * u), holes u; u = r * 2t or get_drm_t(r, t), r = d_other / (d_self + d_other), in fp32
#                        as decisions._ratio_maps / decisions._retime evaluate it.
# The hole test happens inside the kernels, so every value row is decisions.two_branch_rows on the reference's hole mask and its
# unstable set, at the bars gpu_checks.check_glue already holds these entry points to (2e-4 / 2e-5).  The targets are the fp32 sums
# x + flow (softsplat_ref); a finite target beyond the int32 range contributes nothing.  Which path a case takes is chosen and
# asserted from the kernels' host-visible rules as tests/det_common.py restates them (source class, reach, halo variant, records).
RIFE_OP = "rife_splats"
RIFE_BARS = {"flow_reverse": 2e-4, "drm_rife_linear": 2e-5, "drm_rife_nonlinear": 2e-5}
RIFE_EPS = 1e-4
RIFE_FLOW = (("flow_reverse", None),)
RIFE_DRM = (("drm_rife_linear", 0.25), ("drm_rife_nonlinear", 0.3), ("drm_rife_nonlinear", 0.8))
RIFE_MAP = (100, 200)      # 7 x 7 tiles of 32 x 16, the last ragged on both axes (8 columns, 4 rows)
RIFE_SMALL = (48, 96)      # 3 x 3 whole tiles
RIFE_INTERIOR, RIFE_LAST = (2, 2), (6, 6)  # (tx, ty) of the tiles the window rows aim at on RIFE_MAP
RIFE_SIZES = ((1, 1), (1, 40), (17, 1), (5, 7), (16, 32), (17, 33), (15, 31))
RIFE_GROUPS = ("window", "reach", "neighbour", "long", "capacity", "small", "nonfinite", "items")
RIFE_FAR = (float("nan"), float("inf"), float("-inf"), 1e30, -1e30, 3e9, -3e9, 2.0 ** 31, -(2.0 ** 31))
ALONE = 1e4                # an unplanted source of an "alone" map: it leaves the map (and is long: the pre-pass finds no corner)
_RIFE_MEMO = {}            # cases, inputs and references: regenerated from seeds, computed once per process, never written to


class RifeCase(collections.namedtuple("RifeCase", "group name flow drm_flow planted claims")):
    """flow: the [N, 2, H, W] flow of flow_reverse; drm_flow: the splat flow the DRM inputs are constructed for (None: no DRM rows);
    planted: (item, y, x) of the sources whose loss must show; claims: what the CPU suite asserts from the restated rules."""


def _memo(key, fn):
    if key not in _RIFE_MEMO:
        _RIFE_MEMO[key] = fn()
    return _RIFE_MEMO[key]


def rife_u(op, fs, fo, t):
    """u of a DRM entry point in the dtype of its inputs, as the reference evaluates it"""
    from tests import decisions
    _, r = decisions._ratio_maps(fs, fo, RIFE_EPS)
    return decisions._retime(r, t, op == "drm_rife_linear")


def rife_splat_flow(op, fs, fo, t):
    """the fp32 flow an entry point splats along"""
    return fs if op == "flow_reverse" else fs * rife_u(op, fs, fo, t)


def rife_inputs(op, t, flow, planted, seed):
    """(flow_self, flow_other) of a DRM entry point whose splat flow self * u is `flow` up to fp32 rounding (the precedent:
    det_common.other_for): a ratio r0 per pixel -- 0.5 at a planted source, 0.8 .. 0.9 elsewhere, so that a planted source's value
    differs from every other by 0.05 or more at the three timesteps of the rows (the retimed ratio is not monotonic) --, self = flow / u(r0) and an other flow of the length that gives r0."""
    if op == "flow_reverse":
        return flow.contiguous(), None
    from tests import decisions
    n, _, h, w = flow.shape
    r0 = 0.8 + 0.1 * torch.rand(n, 1, h, w, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    for k, y, x in planted:
        r0[k, 0, y, x] = 0.5
    u0 = decisions._retime(r0, t, op == "drm_rife_linear")
    fs = (flow.double() / u0).float()
    ds = (fs[:, 0:1].double() ** 2 + fs[:, 1:].double() ** 2).sqrt() + RIFE_EPS
    d_o = ds * r0 / (1 - r0) - RIFE_EPS
    return fs.contiguous(), torch.cat([d_o, torch.zeros_like(d_o)], 1).float().contiguous()


def _rife_holes(op, t):
    """the reference's hole test in the dtype of its inputs: ones-splat along the splat flow, mode avg, < 0.999"""
    from tests import decisions

    def fn(fs, fo=None):
        f = rife_splat_flow(op, fs, fo, t)
        tgt = _grid32(*f.shape[2:]).to(f.dtype) + f
        f = torch.where(tgt.abs() > 2.0 ** 30, torch.full_like(f, float("inf")), f)  # (beyond int32: no corner, as softsplat_ref)
        return {"hole": oops.softsplat(torch.ones_like(f[:, :1]), f, None, "avg") < decisions.HOLE}
    return fn


def rife_refs(op, t, fs, fo):
    """-> (aligned fp64, fill, hole, unstable) of an entry point on fp32 inputs"""
    from tests import decisions
    _, _, h, w = fs.shape
    if op == "flow_reverse":
        aligned = -2.0 * softsplat_ref(fs, fs, None, "avg")
        fill = torch.full_like(aligned, 2.0 * max(h, w))
        m, u = decisions.unstable(_rife_holes(op, t), [fs])
    else:
        val = rife_u(op, fs, fo, t)
        aligned = softsplat_ref(val, fs * val, None, "avg")
        fill = val
        m, u = decisions.unstable(_rife_holes(op, t), [fs, fo])
    return aligned, fill, m["hole"], u["hole"]


def rife_value(ref):
    """the reference's output: the fill value on its holes, the aligned value elsewhere"""
    aligned, fill, hole, _ = ref
    return torch.where(hole.expand_as(aligned), fill.double().expand_as(aligned), aligned)


def rife_run(ops, dev, op, t, fs, fo):
    if op == "flow_reverse":
        return ops.flow_reverse(fs.to(dev))
    if op == "drm_rife_linear":
        return ops.drm_rife_linear(fs.to(dev), fo.to(dev), t, RIFE_EPS)
    return ops.drm_rife_nonlinear(fs.to(dev), fo.to(dev), t, RIFE_EPS)


def rife_rows(group, name, op, got, ref, extra=""):
    from tests import decisions
    aligned, fill, hole, unst = ref
    fillv = float(fill.flatten()[0])
    rows = []
    for nm, e, tol, x in decisions.two_branch_rows(name, got, aligned, fill, hole, unst, RIFE_BARS[op],
                                                   fill_mask_of=(lambda g: g == fillv) if op == "flow_reverse" else None):
        row = Row(RIFE_OP, nm, e, tol, f"{x} {extra}".strip())
        row.group = group
        rows.append(row)
    return rows


def _rife_bg(kind, n, h, w):
    return torch.full((n, 2, h, w), ALONE) if kind == "alone" else torch.zeros(n, 2, h, w)


def _plant(flow, planted, k, y, x, fx, fy):
    _, _, h, w = flow.shape
    if 0 <= x < w and 0 <= y < h:
        flow[k, 0, y, x], flow[k, 1, y, x] = fx, fy
        planted.append((k, y, x))


def rife_window_cases():
    """Case 1.  Per halo variant R and background, on RIFE_MAP: sources at the window columns tx0 - R, tx0 - R + 1, tx0 + 32 + R - 1 and
    tx0 + 32 + R (one beyond) of an interior tile and of the ragged last one, on x, on y and on the diagonal, with the flows that
    bring the footprint just into the tile's first / last column (-R, -R + 0.25, R - 1.25, just under R - 1) and those that stop one
    short of it.  Nothing else on the map reaches further than R (identity: reach 2; alone: reach 0)."""
    h, w = RIFE_MAP
    out = []
    for R in (4, 8, 16):
        for bg in ("alone", "identity"):
            flows = []
            for exact in (True, False):  # the DRM form keeps clear of the exact bounds: self * u moves a flow by a few ulps
                lo, under = (-float(R), _f32_next(R - 1, 0)) if exact else (-R + 2.0 ** -8, R - 1 - 2.0 ** -8)
                right = ((R - 1, lo), (R - 1, -R + 0.25), (R - 1, -R + 1.0), (R, lo), (R, -R + 0.25))  # (column past the tile, flow)
                left = ((-R + 1, R - 1.25), (-R + 1, under), (-R + 1, R - 2.0), (-R, R - 1.25), (-R, under))  # (column before tx0, flow)
                f, planted = _rife_bg(bg, 1, h, w), []
                for (tx, ty), spare in ((RIFE_INTERIOR, (2, 2)), (RIFE_LAST, (3, 3))):
                    tx0, ty0, sx0, sy0 = tx * 32, ty * 16, spare[0] * 32, spare[1] * 16
                    for k, (c, v) in enumerate(right):
                        _plant(f, planted, 0, sy0 + 1 + k, tx0 + 32 + c, v, 0.0)            # x axis: a row of its own in tile row `spare`
                        _plant(f, planted, 0, ty0 + 16 + c, sx0 + 1 + k, 0.0, v)            # y axis: a column of its own
                    for k, (c, v) in enumerate(left):
                        _plant(f, planted, 0, sy0 + 7 + k, tx0 + c, v, 0.0)
                        _plant(f, planted, 0, ty0 + c, sx0 + 7 + k, 0.0, v)
                    _plant(f, planted, 0, ty0 + 16 + R - 1, tx0 + 32 + R - 1, lo, lo)           # diagonal: onto the far corner pixel
                    _plant(f, planted, 0, ty0 + 16 + R, tx0 + 32 + R, lo, lo)                   # one beyond on both axes
                    _plant(f, planted, 0, ty0 - R + 1, tx0 - R + 1, R - 1.25, R - 1.25)         # onto the near corner pixel
                    _plant(f, planted, 0, ty0 - R, tx0 - R, R - 1.25, R - 1.25)                 # one short on both axes
                flows.append((f, planted))
            assert flows[0][1] == flows[1][1]
            out.append(RifeCase("window", f"window R={R} {bg} {h}x{w}", flows[0][0], flows[1][0], tuple(flows[0][1]),
                                {"variant": R, "tiles": (RIFE_INTERIOR, RIFE_LAST)}))
    return out


REACH_VALUES = (-4.0, _f32_next(-4, -5), 2.75, 3.0, _f32_next(3, 0), -8.0, _f32_next(-8, -9), 6.75, 7.0, _f32_next(7, 0), -16.0,
                _f32_next(-16, -17), 14.75, _f32_next(15, 0), 15.0, -0.0,
                4.5, 8.5, -4.5, -8.5)  # (beyond the issue's list: just past the bounds of the 4- and 8-pixel variants on both sides)


def rife_reach_cases():
    """Case 2.  One source per item on an "alone" 48 x 96 map, so that its tile's reach -- 4, 8, 16, or none: long -- is that source's
    alone.  Every value once in x and once in y only, from the middle of the middle tile and from the place where the far corner of
    the footprint is the first column (row) of the next tile, or the last one of the tile before: the pixel a halo chosen one too
    small does not bring in."""
    h, w = RIFE_SMALL
    n = 4 * len(REACH_VALUES)
    f, planted = _rife_bg("alone", n, h, w), []
    for k, v in enumerate(REACH_VALUES):
        _plant(f, planted, 4 * k, 24, 48, v, 0.0)
        _plant(f, planted, 4 * k + 1, 24, 48, 0.0, v)
        _plant(f, planted, 4 * k + 2, 24, 31 - math.ceil(v) if v < 0 else 64 - (math.floor(v) + 1), v, 0.0)  # onto column 31 / corner on 64
        _plant(f, planted, 4 * k + 3, 15 - math.ceil(v) if v < 0 else 32 - (math.floor(v) + 1), 48, 0.0, v)  # onto row 15 / corner on 32
    assert len(planted) == n
    return [RifeCase("reach", f"reach rounding N={n} alone {h}x{w}", f, None, tuple(planted), {"values": REACH_VALUES})]


def rife_neighbour_cases():
    """Case 3.  Items 0-3: the middle tile of a 3 x 3 tile map is all holes (reach 0) and its right, lower, diagonal or upper-left
    neighbour holds one source of reach 16 that lands on the quiet tile's corner pixel; items 4, 5: the quiet tile is a corner tile
    of the map (some neighbours do not exist); item 6, the mirror: the middle tile's sources have reach 16 and land inside their own
    tile, so that the eight neighbours scan 64 x 48 windows and find nothing."""
    h, w = RIFE_SMALL
    f, planted = _rife_bg("alone", 7, h, w), []
    lo = -16.0
    _plant(f, planted, 0, 31, 79, lo, 0.0)      # right neighbour (2, 1) -> (63, 31), the far corner of tile (1, 1)
    _plant(f, planted, 1, 47, 63, 0.0, lo)      # lower neighbour (1, 2)
    _plant(f, planted, 2, 47, 79, lo, lo)       # diagonal (2, 2)
    _plant(f, planted, 3, 1, 17, 14.75, 14.75)  # upper left (0, 0) -> (31.75, 15.75): the near corner (32, 16)
    _plant(f, planted, 4, 17, 49, 14.75, 14.75)  # quiet corner tile (2, 2): from (1, 1) onto (64, 32)
    _plant(f, planted, 5, 31, 47, lo, lo)       # quiet corner tile (0, 0): from (1, 1) onto its far corner (31, 15)
    _plant(f, planted, 6, 17, 33, 14.75, 10.5)
    _plant(f, planted, 6, 30, 62, lo, -12.0)
    quiet = {0: (1, 1), 1: (1, 1), 2: (1, 1), 3: (1, 1), 4: (2, 2), 5: (0, 0)}
    return [RifeCase("neighbour", f"neighbour reach N=7 alone {h}x{w}", f, None, tuple(planted), {"quiet": quiet, "mirror": 6})]


def rife_long_cases():
    """Case 4.  Long sources on an "alone" map whose footprint has exactly one corner inside the map, one per map corner, and the
    short-only flow of the call that follows on the same workspace."""
    h, w = RIFE_MAP
    f, planted = _rife_bg("alone", 1, h, w), []
    for y, x, tx, ty in ((30, 40, -0.5, -0.5), (31, 150, w - 0.5, -0.5), (70, 41, -0.5, h - 0.5), (71, 151, w - 0.5, h - 0.5)):
        _plant(f, planted, 0, y, x, tx - x, ty - y)
    quiet = cases.rnd((1, 2, h, w), 3400, 1.0).clamp(-2.9, 2.9)
    return [RifeCase("long", f"long, one corner inside, alone {h}x{w}", f, f.clone(), tuple(planted), {"long": len(planted)}),
            RifeCase("long", f"short only, after the long call {h}x{w}", quiet, quiet.clone(), (), {"long": 0})]


PINCH = (2, 2)  # (tx, ty) of the tile the capacity rows contract a patch into
CAPACITY_TOTALS = (("CAP-1", 1535, False, False), ("CAP", 1536, False, False), ("CAP+1", 1537, False, True), ("CAP+1 and a long source", 1537, True, True),
                   ("1.5 CAP", 2304, False, True), ("1.5 CAP and a long source", 2304, True, True))  # (label, records, long source, DRM rows)


def pinch_flow(h, w, tile=PINCH, n=1):
    """[n, 2, h, w] "alone" map with a 67 x 50 patch contracted about the centre of `tile`, by 0.45 in x and 0.6 in y: every source of
    the patch is short (|f| < 14.9) and lands within 14.9 columns and 9.8 rows of the centre -- inside the tile in x, and over its
    upper and lower edge in y, so that the patch holds records that straddle the edge.  About 2900 records of `tile`."""
    from tests import det_common
    cx, cy = tile[0] * det_common.TX + 15.5, tile[1] * det_common.TY + 7.5
    g = _grid32(h, w)
    f = _rife_bg("alone", n, h, w)
    py, px = slice(int(cy - 24.5), int(cy - 24.5) + 50), slice(int(cx - 32.5), int(cx - 32.5) + 67)
    f[:, 0, py, px] = -0.45 * (g[0, py, px] - cx)
    f[:, 1, py, px] = -0.6 * (g[1, py, px] - cy)
    return f


def _pinch_to(op, t, fs, fo, tile, total, seed):
    """Sources of `tile`'s records taken out (sent off the map) one by one, in a seeded order and only those that are records of no
    other tile, until the restated record total of the tile is `total`; in place."""
    from tests import det_common
    flow = rife_splat_flow(op, fs, fo, t)
    have = int(det_common.tile_record_totals(flow)[0, tile[1], tile[0]])
    assert have >= total, (have, total)
    kx, ky, ok = det_common.record_keys(flow)
    tx0, ty0 = tile[0] * det_common.TX, tile[1] * det_common.TY
    inner = ok[0] & (kx[0] >= tx0) & (kx[0] <= tx0 + 30) & (ky[0] >= ty0) & (ky[0] <= ty0 + 14)  # on no other tile's key grid
    idx = inner.flatten().nonzero()[:, 0]
    idx = idx[torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(seed))][:have - total]
    w = fs.shape[3]
    if op == "flow_reverse":
        fs[0, :, idx // w, idx % w] = ALONE
    else:  # self == other: r = 0.5, u about t, and self * u still leaves the map
        fs[0, :, idx // w, idx % w] = ALONE / 0.1
        fo[0, :, idx // w, idx % w] = ALONE / 0.1
    assert int(det_common.tile_record_totals(rife_splat_flow(op, fs, fo, t))[0, tile[1], tile[0]]) == total


def capacity_inputs(label, op, t):
    """inputs of one capacity row: the pinch, a long source onto the pinch tile where the row names one, and sources removed until
    the tile's records are exactly those the row claims -- counted on the flow the entry point splats along"""
    def make():
        h, w = RIFE_MAP
        _, total, with_long, _ = next(c for c in CAPACITY_TOTALS if c[0] == label)
        f = pinch_flow(h, w)
        planted = []
        if with_long:
            _plant(f, planted, 0, 90, 170, (PINCH[0] * 32 + 6.5) - 170, (PINCH[1] * 16 + 8.5) - 90)
        fs, fo = rife_inputs(op, t, f, planted, 3500)
        _pinch_to(op, t, fs, fo, PINCH, total, 3501)
        return fs, fo, tuple(planted)
    return _memo(("capacity", label, op, t), make)


def rife_small_flow(h, w, seed):
    """sigma = 2 noise, and sources whose x (then y) target walks over -1, 0, W - 1, W and their fp32 neighbours (border_flow's walk,
    on the sources a small map has): asserted as the fp32 sums they are"""
    f = cases.rnd((1, 2, h, w), seed, 2.0)
    want = {}
    for axis, size in ((0, w), (1, h)):
        k = 0
        for edge in (-1.0, 0.0, size - 1.0, float(size)):
            for side in (0, -1, 1):  # the integer, then the nearest targets this source can have below and above it
                p = (k * 5 + 17 * axis + 2) % (h * w)
                y, x = p // w, p % w
                tgt = edge if side == 0 else _f32_next(edge, edge + side)
                f[0, axis, y, x] = tgt - (x, y)[axis]
                want[(axis, y, x)] = (edge, side, tgt)
                k += 1
    tg = _grid32(h, w) + f[0]
    hit = 0
    for (axis, y, x), (edge, side, tgt) in want.items():  # (a neighbour finer than the source's own flow can express lands on the edge itself)
        got = float(tg[axis, y, x])
        assert got == tgt or got == edge, (h, w, axis, y, x, edge, side, got)
        hit += got == tgt and side != 0
    assert hit >= min(3, h * w - 1), (h, w, hit)
    return f


def rife_small_cases():
    """Case 6.  Maps smaller than a tile, one tile exactly, and one pixel more / less than a tile on both axes."""
    return [RifeCase("small", f"small {h}x{w}", rife_small_flow(h, w, 3600 + k), None, (), {}) for k, (h, w) in enumerate(RIFE_SIZES)]


def rife_nonfinite_cases():
    """Case 7.  NaN, +-inf, +-1e30, +-3e9 and +-2^31 in either component, on sigma = 2 noise: at the corner pixels of tiles and at
    the border pixels a border tile's window clamps its out-of-map positions to."""
    h, w = RIFE_SMALL
    f = cases.rnd((1, 2, h, w), 3700, 2.0)
    spots = ((16, 32), (31, 63), (15, 31), (32, 64), (0, 0), (47, 95), (0, 95), (47, 0), (16, 0), (31, 95), (0, 32), (47, 63),  # (y, x)
             (15, 0), (32, 95), (0, 31), (47, 64), (20, 0), (25, 95))
    assert len(spots) == 2 * len(RIFE_FAR)
    for k, (y, x) in enumerate(spots):
        f[0, k % 2, y, x] = RIFE_FAR[k // 2]
    return [RifeCase("nonfinite", f"NaN inf 1e30 3e9 2^31 {h}x{w}", f, None, (), {"spots": spots})]


ITEMS = 8
ITEM_REACH16 = ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (5, 5), (6, 5))  # (tx, ty) of item k's reach-16 tile; item k + 1's quiet tile
ITEM_PINCH = ((1, 3), (2, 4), (3, 3), (4, 4), (1, 4), (2, 3), (3, 2), (4, 2))
ITEM_FP64 = (0, 3, 7)
ITEM_T = {"drm_rife_linear": (0.25, 0.2, 0.3, 0.35, 0.4, 0.45, 0.55, 0.6), "drm_rife_nonlinear": (0.3, 0.8, 0.25, 0.4, 0.6, 0.7, 0.35, 0.65)}


def rife_item_flow():
    """Case 8.  [8, 2, 100, 200]: per item its own reach-4 noise, a pinch of more than kCAP records, a 6 x 6 block of 40-pixel flows
    and a reach-16 tile, each at another place; the reach-16 tile of item k - 1 is all NaN (reach 0, no flag) in item k."""
    def make():
        h, w = RIFE_MAP
        f = cases.rnd((ITEMS, 2, h, w), 3800, 1.0).clamp(-2.9, 2.9)
        planted = []
        for k in range(ITEMS):
            p = pinch_flow(h, w, ITEM_PINCH[k])[0]
            patch = p[0] != ALONE
            f[k] = torch.where(patch, p, f[k])
            f[k, 0, 84:90, 4 + 12 * k:10 + 12 * k] = 40.0
            tx0, ty0 = ITEM_REACH16[k][0] * 32, ITEM_REACH16[k][1] * 16
            qx0, qy0 = ITEM_REACH16[k - 1][0] * 32, ITEM_REACH16[k - 1][1] * 16
            f[k, :, qy0:qy0 + 16, qx0:qx0 + 32] = float("nan")
            _plant(f, planted, k, ty0 + 5, min(tx0 + 20, w - 1), -16.0, 0.0)
            _plant(f, planted, k, 86, 6 + 12 * k, 40.0, 0.0)
        return f, tuple(planted)
    return _memo("items", make)


def rife_cases(groups=RIFE_GROUPS):
    """the table of cases 1-4, 6 and 7 (one flow per case); the capacity and item rows build their inputs per entry point"""
    def make():
        return rife_window_cases() + rife_reach_cases() + rife_neighbour_cases() + rife_long_cases() + rife_small_cases() + rife_nonfinite_cases()
    return [c for c in _memo("cases", make) if c.group in groups]


def rife_case_inputs(case, op, t):
    def make():
        if op == "flow_reverse":
            return case.flow.contiguous(), None
        return rife_inputs(op, t, case.drm_flow, case.planted, 3300)
    return _memo(("inputs", case.name, op, t), make)


def rife_case_refs(name, op, t, fs, fo):
    return _memo(("refs", name, op, t), lambda: rife_refs(op, t, fs, fo))


def rife_workspace(ops, dev):
    """the zeroed buffer the fused entry points share, as allocated by the calls made so far"""
    return ops._zero_workspace(dev, 1)


def _ws_row(group, name, ops, dev):
    from tests import det_common
    ws = rife_workspace(ops, dev)
    row = Row(RIFE_OP, f"{name}: non-zero workspace words past the reach map", float((ws[det_common.REACH_WORDS:] != 0).sum()), 0.0,
              f"{ws.numel() - det_common.REACH_WORDS} words")
    row.group = group
    return row


def _item_rows(rows, ops, dev, tag):
    """Case 8: the single-tensor form at N = 8 and the two batch forms with 8 jobs, against fp64 on items 0, 3, 7 and against the
    N = 1 calls on every item"""
    f, planted = rife_item_flow()
    for op in ("flow_reverse", "drm_rife_linear", "drm_rife_nonlinear"):
        if op == "flow_reverse":
            ins = [(f[k:k + 1].contiguous(), None, None) for k in range(ITEMS)]
            got = ops.flow_reverse(f.to(dev))
            got = [got[k:k + 1] for k in range(ITEMS)]
        else:
            def make(op=op):
                return [rife_inputs(op, ITEM_T[op][k], f[k:k + 1], [(0, y, x) for i, y, x in planted if i == k], 3810 + k) + (ITEM_T[op][k],)
                        for k in range(ITEMS)]
            ins = _memo(("item inputs", op), make)
            many = ops.drm_rife_linear_many if op == "drm_rife_linear" else ops.drm_rife_nonlinear_many
            got = many([(a.to(dev), b.to(dev), t) for a, b, t in ins], RIFE_EPS)
        worst = 0.0
        for k, (a, b, t) in enumerate(ins):
            one = rife_run(ops, dev, op, t, a, b)
            worst = max(worst, _err(got[k], one.double()))
            if k in ITEM_FP64:
                name = f"{op} item {k} of {ITEMS}" + ("" if t is None else f" t={t}")
                rows += rife_rows("items", f"{name}{tag}", op, got[k], rife_case_refs(f"item {k}", op, t, a, b))
        row = Row(RIFE_OP, f"{op} {ITEMS} items vs the N=1 calls{tag}", worst, RIFE_BARS[op], "")
        row.group = "items"
        rows.append(row)


def check_rife_splats(dev, ops=None, groups=RIFE_GROUPS, modes=(False, True)):
    """Cases 1-8 of the fused RIFE splats and the t_dev row, in the default and in the deterministic mode, against the same references
    at the same bars: window edges per halo variant, reach rounding, neighbour reach, long sources and the flags, the record capacity,
    small and ragged maps, non-finite and far flows, items."""
    ops = ops or default_ops()
    rows = []
    was = ops.set_deterministic(False)
    try:
        for det in modes:
            ops.set_deterministic(det)
            tag = " det" if det else ""
            for case in rife_cases(groups):
                for op, t in RIFE_FLOW + (RIFE_DRM if case.drm_flow is not None else ()):
                    fs, fo = rife_case_inputs(case, op, t)
                    name = f"{op}{'' if t is None else f' t={t}'} {case.name}{tag}"
                    got = rife_run(ops, dev, op, t, fs, fo)
                    rows += rife_rows(case.group, name, op, got, rife_case_refs(case.name, op, t, fs, fo))
                    if case.group == "long":  # the accumulators and the flags behind them are zero again after every call
                        rows.append(_ws_row("long", name, ops, dev))
            if "capacity" in groups:
                for label, total, with_long, drm in CAPACITY_TOTALS:
                    for op, t in RIFE_FLOW + (RIFE_DRM if drm else ()):
                        fs, fo, _ = capacity_inputs(label, op, t)
                        name = f"{op}{'' if t is None else f' t={t}'} capacity {label}{tag}"
                        got = rife_run(ops, dev, op, t, fs, fo)
                        rows += rife_rows("capacity", name, op, got, rife_case_refs(f"capacity {label}", op, t, fs, fo), f"records={total}")
                        rows.append(_ws_row("capacity", name, ops, dev))
            if "items" in groups:
                _item_rows(rows, ops, dev, tag)
            if "long" in groups and not det:  # case 10: t from device memory == t from the host, bit for bit
                case = rife_cases(("long",))[0]
                fs, fo = rife_case_inputs(case, "drm_rife_linear", 0.25)
                a, b = fs.to(dev), fo.to(dev)
                host = ops.drm_rife_linear(a, b, 0.25, RIFE_EPS)
                devt = ops.drm_rife_linear(a, b, 0.75, RIFE_EPS, t_dev=torch.tensor([0.25]).to(dev))
                row = exact_row(RIFE_OP, "drm_rife_linear t_dev == host t", devt, host)
                row.group = "long"
                rows.append(row)
    finally:
        ops.set_deterministic(was)
    return rows


# ---- case 9: launches without the reach map
NOMAP_W = 3  # one tile column; the smallest width of the issue's range, i.e. the fewest pixels


def nomap_geometry(reach_words, with_map):
    """(N, H) with N * tiles == reach_words (the map is used) or one tile row more per item (skipped); N is the largest power of two
    that keeps H below 2^15 + 16 rows and the grid's y below 65536"""
    n = max(4, reach_words >> 11)
    ty = reach_words // n
    assert n * ty == reach_words
    return (n, ty * 16 - 3) if with_map else (n, ty * 16 + 5)


def nomap_flow(n, h, seed):
    """[n, 2, h, NOMAP_W]: noise of reach at most 4, and in the first, a middle and the last item a few long and non-finite sources"""
    w = NOMAP_W
    f = torch.randn(n, 2, h, w, generator=torch.Generator().manual_seed(seed)).clamp(-2.9, 2.9)
    f[:, 0] *= 0.3
    planted = []
    for k in (0, n // 2, n - 1):
        _plant(f, planted, k, 5, 1, 0.25, 40.5)
        _plant(f, planted, k, h - 3, 0, 1.5, -60.75)  # (flows stay below 2^7: the 2e-4 bar is absolute, and an fp32 ulp of a longer flow is not below it)
        _plant(f, planted, k, h // 2, 2, -1.25, 17.0)
        _plant(f, planted, k, 79, 1, 0.0, -16.0)      # reach 16, from the last row of a tile's 16-pixel window onto its last row
        _plant(f, planted, k, 113, 1, 0.25, 14.75)    # reach 16, from the second row of the window onto the first row of tile 8
        f[k, 0, 9, 1], f[k, 1, h - 9, 2], f[k, 0, h // 2 + 3, 0] = float("nan"), float("inf"), 3e9
    return f, tuple(planted)


def check_rife_splats_nomap(dev, ops=None, reach_words=None):
    """Case 9.  flow_reverse on one tile column (W = 3) with N * tiles == REACH_WORDS -- the largest launch that uses the reach map: noise
    of reach <= 4 takes the 40 x 24 windows -- and with one tile row more per item: the map is skipped and every tile scans 64 x 48.
    Against fp64 on the first, a middle and the last item, against the same entry point on two chunks of N / 2 items (which use the
    map) on every item, and in deterministic mode bit for bit against the chunks; each launch once with the reach words set to 0 and
    once to 0x7f7f7f7f beforehand.  At REACH_WORDS = 2^18: N = 128, H = 32765 / 32773, 12.6 M pixels; on the device 101 MB of flow, as
    much output and the same again for the chunks' results, and a workspace of 152 MB (303 MB in deterministic mode): 0.7 GB.
    reach_words: the CPU suite runs the same rows on a stand-in with a smaller map."""
    from tests import det_common
    ops = ops or default_ops()
    rw = reach_words or det_common.REACH_WORDS
    rows = []
    was = ops.set_deterministic(False)
    try:
        for with_map in (True, False):
            n, h = nomap_geometry(rw, with_map)
            f, _ = _memo(("nomap", rw, with_map), lambda: nomap_flow(n, h, 3900 + int(with_map)))
            fd = f.to(dev)
            what = f"N={n} {h}x{NOMAP_W} tiles={n * ((h + 15) // 16)} ({'with' if with_map else 'without'} the reach map)"
            for det in (False, True):
                ops.set_deterministic(det)
                tag = " det" if det else ""
                chunks = torch.cat([ops.flow_reverse(fd[:n // 2].contiguous()), ops.flow_reverse(fd[n // 2:].contiguous())], 0)
                ops.flow_reverse(fd)  # (the workspace of this geometry and mode is allocated from here on)
                for fillv in (0, 0x7f7f7f7f):
                    rife_workspace(ops, dev)[:rw].view(torch.int32).fill_(fillv)
                    got = ops.flow_reverse(fd)
                    name = f"flow_reverse {what} reach words {fillv:#x}{tag}"
                    for k in (0, n // 2, n - 1):
                        a = f[k:k + 1].contiguous()
                        rows += rife_rows("nomap", f"{name} item {k}", "flow_reverse", got[k:k + 1], rife_case_refs(f"nomap {rw} {with_map} {k}", "flow_reverse", None, a, None))
                    if det:
                        row = exact_row(RIFE_OP, f"{name}: == two chunks of N/2", got, chunks)
                    else:
                        row = Row(RIFE_OP, f"{name}: vs two chunks of N/2", _err(got, chunks.double()), RIFE_BARS["flow_reverse"], "")
                    row.group = "nomap"
                    rows += [row, _ws_row("nomap", name, ops, dev)]
                    del got
                del chunks
    finally:
        ops.set_deterministic(was)
    return rows


SPLAT_CHECKS = (check_softsplat, check_softsplat_scan, check_softsplat_big)  # the generic splat's families, for tests that take them together
CHECKS = (  # (section title, check): one operator family each
    ("op softmax_rows_", check_softmax_rows), ("op instance_norm", check_instance_norm), ("op conv_direct", check_conv_direct),
    ("op local_corr_flow", check_local_corr_flow), ("op local_attn_flow", check_local_attn_flow),
    ("op convex_upsample", check_convex_upsample), ("op flow_warp", check_flow_warp), ("op backwarp", check_backwarp),
    ("op resize_bilinear_ac", check_resize_bilinear_ac), ("op layernorm", check_layernorm), ("op gelu", check_gelu), ("op bmm", check_bmm),
    ("op pointwise", check_pointwise), ("op layouts", check_layouts), ("op hole tests", check_hole_tests), ("op drm", check_drm),
    ("op metric_input", check_metric_input), ("op softsplat", check_softsplat), ("op softsplat scan geometry", check_softsplat_scan),
    ("op softsplat big map", check_softsplat_big), ("op resize_bilinear_scale", check_resize_scale), ("op flow_distance", check_flow_distance),
    ("op stage input, first stage", check_stage_input_first), ("op stage input, warped", check_stage_input_warped),
    ("op stage input + conv0[0] fused", check_stage_conv_fused), ("op flow update", check_flow_update), ("op warp + blend", check_warp_blend),
    ("op conv epilogue forms", check_conv_forms_all), ("op window attention edges", check_window_attention_edges),
    ("op global_expect2 edges", check_global_expect2_edges), ("op linear_split edges", check_linear_split_edges),
    ("op fused encoder", check_head_fused), ("op fused RIFE splats", check_rife_splats))
GLUE_CHECKS = (check_stage_input_first, check_stage_input_warped, check_stage_conv_fused, check_flow_update, check_warp_blend)
