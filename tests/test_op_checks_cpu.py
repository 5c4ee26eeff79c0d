"""CPU (-m "not gpu"): the per-operator checks of tests/op_checks.py CAN fail, and their references are right.

The "implementation under test" here is a torch-fp32 stand-in for drba_amd.ops, written tap by tap the way the kernels are
(explicit window loops, explicit bilinear gathers, explicit index arithmetic; the forward splat as a key per source, the
sources ordered by key and the outputs summing their four segments; the IFNet stage glue with a source index and weight per
axis, 2 x 2 gathers at clamped coordinates and the running flow summed term by term; IFNet's encoder as the four layers with both
output layouts taken from the same values; the fused RIFE splats as a reach map, a halo variant per tile, a window test per
(source, corner) pair and a record capacity per tile) -- not with the unfold / grid_sample / F.interpolate /
corner-by-corner scatter forms the fp64 references use -- so that two independent statements of every formula meet:
  1. every fp64 reference agrees with the fp32 oracle / torch form of the same formula within fp32 roundoff (the measured
     floor of each row is bounded by a figure derived from the number format and the operation's conditioning);
  2. the stand-in passes every row;
  3. with one planted defect at a time (a one-line variant of one stand-in function) the row meant to catch it fails, and
     only rows of that operator fail."""
import pytest
import torch
import torch.nn.functional as F

from oracle import drm as odrm
from tests import det_common, op_checks

CPU = torch.device("cpu")
EPS32 = 2.0 ** -24


# ----------------------------------------------------------------------------------------- the stand-in
def _softmax_rows_(scores, scale, mask=None, defect=False):
    for i in range(scores.shape[0]):
        s = scores[i] / scale
        if mask is not None:
            if not (defect and i >= mask.shape[0]):
                s = s + mask[i % mask.shape[0]]
        s = s - s.max(dim=-1, keepdim=True).values
        e = s.exp()
        scores[i] = e / e.sum(dim=-1, keepdim=True)
    return scores


def _instance_norm(x, relu=False, eps=1e-5, defect=False):
    hw = x.shape[2] * x.shape[3]
    mean = x.sum((2, 3), keepdim=True) / hw
    m2 = ((x - mean) ** 2).sum((2, 3), keepdim=True)
    y = (x - mean) / torch.sqrt(m2 / ((hw - 1) if defect else hw) + eps)
    return y.clamp(min=0) if relu else y


def _conv_direct(x, w, bias, stride, pad, defect=False):
    if defect and bias is not None:
        bias = bias.clone()
        bias[16:] = 0.0
    return F.conv2d(x, w, bias, stride=stride, padding=pad)


def _window(t, r, dy, dx):
    """t [.., h, w] moved by (dy, dx) with zeros from outside the image"""
    h, w = t.shape[-2:]
    return F.pad(t, (r, r, r, r))[..., r + dy:r + dy + h, r + dx:r + dx + w]


def _local_corr_flow(f0, f1, radius):
    _, c, h, w = f0.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    sc, cx, cy = [], [], []
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            inside = (ys + dy >= 0) & (ys + dy < h) & (xs + dx >= 0) & (xs + dx < w)
            s = (f0[0] * _window(f1[0], radius, dy, dx)).sum(0) / c ** 0.5
            sc.append(torch.where(inside, s, torch.full_like(s, -1e4)))
            cx.append(xs + dx)
            cy.append(ys + dy)
    p = torch.softmax(torch.stack(sc), 0)
    return torch.stack([(p * torch.stack(cx)).sum(0) - xs, (p * torch.stack(cy)).sum(0) - ys])[None]


def _local_attn_flow(q_tok, k_tok, flow, radius, defect=False):
    _, _, h, w = flow.shape
    c = q_tok.shape[-1]
    q, k = q_tok.reshape(h, w, c).permute(2, 0, 1), k_tok.reshape(h, w, c).permute(2, 0, 1)
    inside_src = torch.ones(h, w)
    sc, fl = [], []
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            s = (q * _window(k, radius, dy, dx)).sum(0) / c ** 0.5  # an out-of-image key is a zero vector: score 0
            if defect:
                s = torch.where(_window(inside_src, radius, dy, dx) > 0, s, torch.full_like(s, float("-inf")))
            sc.append(s)
            fl.append(_window(flow[0], radius, dy, dx))
    p = torch.softmax(torch.stack(sc), 0)
    return (p.unsqueeze(1) * torch.stack(fl)).sum(0)[None]


def _convex_upsample(mask, flow, factor, defect=False):
    _, _, h, w = flow.shape
    k = factor
    m = torch.softmax(mask.view(9, k, k, h, w), 0)  # [tap, ii, jj, y, x]
    if defect:
        m = m.transpose(1, 2)
    up = torch.zeros(2, k, k, h, w)
    for t in range(9):
        up += m[t].unsqueeze(0) * (k * _window(flow[0], 1, t // 3 - 1, t % 3 - 1)).view(2, 1, 1, h, w)
    return up.permute(0, 3, 1, 4, 2).reshape(1, 2, k * h, k * w)  # [c, y, ii, x, jj]


def _bilinear(x, sx, sy, padding, edge=False):
    """x [N, C, H, W] sampled at pixel coordinates sx, sy [N, H, W]: four bounds-checked taps (zeros) or clamped coordinates
    (border); a non-finite coordinate has no tap inside the image.  edge (planted): a sample in the last column takes its left
    tap from the column before it, as a pair load based at W - 2 invites."""
    n, c, h, w = x.shape
    if padding == "border":
        sx, sy = sx.clamp(0, w - 1), sy.clamp(0, h - 1)
    fin = torch.isfinite(sx) & torch.isfinite(sy)
    sx, sy = torch.where(fin, sx, torch.full_like(sx, -9.0)), torch.where(fin, sy, torch.full_like(sy, -9.0))
    x0, y0 = sx.floor(), sy.floor()
    wx1, wy1 = sx - x0, sy - y0
    out = torch.zeros_like(x)
    flat = x.reshape(n, c, h * w)
    for dx, dy, wgt in ((0, 0, (1 - wx1) * (1 - wy1)), (1, 0, wx1 * (1 - wy1)), (0, 1, (1 - wx1) * wy1), (1, 1, wx1 * wy1)):
        xi, yi = x0 + dx, y0 + dy
        if edge and dx == 0:
            xi = torch.where(x0 >= w - 1, x0 - 1, xi)
        ok = fin & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long().view(n, 1, h * w).expand(n, c, h * w)
        out += flat.gather(2, idx).view(n, c, h, w) * (wgt * ok).unsqueeze(1)
    return out


def _grid(n, h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return xs.expand(n, h, w), ys.expand(n, h, w)


def _flow_warp(x, flow):
    n, _, h, w = x.shape
    xs, ys = _grid(n, h, w)
    gx, gy = 2 * (xs + flow[:, 0]) / (w - 1) - 1, 2 * (ys + flow[:, 1]) / (h - 1) - 1
    return _bilinear(x, (gx + 1) * ((w - 1) / 2), (gy + 1) * ((h - 1) / 2), "zeros")


def _backwarp(x, flow, padding="border"):
    n, _, h, w = x.shape
    gx = torch.linspace(-1.0, 1.0, w).view(1, 1, w) + flow[:, 0] / ((w - 1.0) / 2.0)
    gy = torch.linspace(-1.0, 1.0, h).view(1, h, 1) + flow[:, 1] / ((h - 1.0) / 2.0)
    return _bilinear(x, (gx + 1) * ((w - 1.0) / 2.0), (gy + 1) * ((h - 1.0) / 2.0), padding)


def _resize_bilinear_ac(x, size, mul=1.0, defect=False):
    if defect:
        return F.interpolate(x, size=size, mode="bilinear", align_corners=False) * mul
    (hi, wi), (ho, wo) = x.shape[2:], size

    def axis(n_in, n_out):
        s = torch.arange(n_out, dtype=torch.float32) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        i0 = s.floor().clamp(max=n_in - 1)
        return i0.long(), (i0 + 1).clamp(max=n_in - 1).long(), s - i0

    y0, y1, ly = axis(hi, ho)
    x0, x1, lx = axis(wi, wo)
    ly = ly.view(-1, 1)
    top = x[:, :, y0][:, :, :, x0] * (1 - lx) + x[:, :, y0][:, :, :, x1] * lx
    bot = x[:, :, y1][:, :, :, x0] * (1 - lx) + x[:, :, y1][:, :, :, x1] * lx
    return (top * (1 - ly) + bot * ly) * mul


def _layernorm(x, w, b, residual=None, eps=1e-5):
    mean = x.mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps) * w + b
    return y if residual is None else residual + y


def _timestep_fix(t0, t1, c0, c1, defect=False):
    bad = ((c0 <= 0.999) | (c1 <= 0.999)) if defect else ((c0 < 0.999) | (c1 < 0.999))
    return torch.where(bad, torch.ones_like(t0), t0), torch.where(bad, torch.ones_like(t1), t1)


def _drm_ratio(f10, f12, eps):
    a, b = (f10[:, 0:1] ** 2 + f10[:, 1:2] ** 2).sqrt(), (f12[:, 0:1] ** 2 + f12[:, 1:2] ** 2).sqrt()
    if eps:
        a, b = a + eps, b + eps
    return a / (a + b), b / (a + b)


def _retime_regrouped(drm, t, precision):
    """oracle.drm.drm_to_t with every map update regrouped (x - (x - l) f -> x (1 - f) + l f): equal in exact arithmetic, and
    within an ulp or two in fp32 -- what a tolerance would wave through and the bit-exact row must not"""
    x, lo, hi = 0.5, 0.0, 1.0
    xm, fm = drm.clone(), drm.clone()
    lom, him = xm * 0, xm * 0 + 1
    while abs(x - t) > precision:
        if x > t:
            hi, x, him = x, x - (x - lo) * 0.5, xm.clone()
            xm = xm * (1 - fm) + lom * fm
        if x < t:
            lo, x, lom = x, x + (hi - x) * 0.5, xm.clone()
            xm = xm * (1 - fm) + him * fm
    return xm


def _metric_input(img0, img1, f01, f10, defect=False):
    _, _, h, w = img0.shape
    m0 = (img0 - _backwarp(img1, f01, "zeros")).abs().sum(1, keepdim=True) / 3
    m1 = (img1 - _backwarp(img0, f10, "zeros")).abs().sum(1, keepdim=True) / 3
    hx, hy = (w - 1.0) / 2.0, (h - 1.0) / 2.0
    norm = lambda f: (f[:, 0:1] ** 2 + f[:, 1:2] ** 2).sqrt()  # noqa: E731
    thr = 0.01 * (norm(f01) + norm(f10)) + (0.49 if defect else 0.5)
    df, db = norm(f01 + _flow_warp(f10, f01)), norm(f10 + _flow_warp(f01, f10))
    occ = lambda d: ((d >= thr) if defect else (d > thr)).float()  # noqa: E731
    return torch.cat([img0, img1, -m0, -m1, f01[:, 0:1] / hx, f01[:, 1:2] / hy, f10[:, 0:1] / hx, f10[:, 1:2] / hy, occ(df), occ(db)], 1)


def _softsplat(x, flow, metric, mode, out=None, keep_quad=False, defect=None):
    """The generic splat in the kernels' form: one key per source (the pixel its 2 x 2 footprint starts at, on the
    (H + 1) x (W + 1) grid of every image), the sources ordered by key, and every output summing the records of the four keys
    that cover it, footprint row by footprint row, right key before left -- weight = m * (wx * wy), value * weight, the
    normaliser the sum of the weights.  (The oracle scatters corner by corner in source order, value * m first.)"""
    main, _, sub = mode.partition("-")
    n, c, h, w = x.shape
    if defect == "base_of_image0":  # image n reads the records of image 0
        flow = flow[0:1].expand(n, 2, h, w)
        metric = None if metric is None else metric[0:1].expand(n, 1, h, w)
    if defect == "tail_repeats" and c == 17:
        x = torch.cat([x[:, :16], x[:, 15:16]], 1)
    xs, ys = _grid(n, h, w)
    X, Y = xs + flow[:, 0], ys + flow[:, 1]
    fx, fy = X.floor(), Y.floor()
    first = 0.0 if defect == "no_minus1" else -1.0
    ok = torch.isfinite(X) & torch.isfinite(Y) & (fx >= first) & (fx <= w - 1) & (fy >= first) & (fy <= h - 1)
    img = torch.arange(n).view(n, 1, 1).expand(n, h, w)[ok]
    src = torch.arange(h * w).view(1, h, w).expand(n, h, w)[ok]
    m = torch.ones(n, h, w) if main in ("sum", "avg") else (metric[:, 0] if main == "linear" else metric[:, 0].exp())
    X, Y, fx, fy, m = X[ok], Y[ok], fx[ok], fy[ok], m[ok]
    key = img * ((h + 1) * (w + 1)) + (fy.long() + 1) * (w + 1) + (fx.long() + 1)
    order = torch.sort(key, stable=True).indices
    if defect == "lost_keys":
        order = order[key[order] < (1 << 20)]
    img, src, X, Y, fx, fy, m = (t[order] for t in (img, src, X, Y, fx, fy, m))
    vals = x.permute(0, 2, 3, 1).reshape(n * h * w, c)[img * (h * w) + src]
    acc, nrm = torch.zeros(n * h * w, c), torch.zeros(n * h * w)
    for dy in (0, 1):
        for dx in (1, 0):
            wgt = m * ((X - fx if dx else (fx + 1) - X) * (Y - fy if dy else (fy + 1) - Y))
            px, py = fx.long() + dx, fy.long() + dy
            inb = (px >= 0) & (px < w) & (py >= 0) & (py < h)
            lin = (img * (h * w) + py * w + px)[inb]
            nrm.index_add_(0, lin, wgt[inb])
            acc.index_add_(0, lin, vals[inb] * wgt[inb].unsqueeze(1))
    if main != "sum":
        if sub in ("", "addeps") or defect == "zeroeps_as_addeps":
            nrm = nrm + 0.0000001
        elif sub == "zeroeps":
            nrm = torch.where(nrm == 0, torch.ones_like(nrm), nrm)
        else:
            nrm = nrm.clamp(min=0.0000001)
        acc = acc / nrm.unsqueeze(1)
    res = acc.view(n, h, w, c).permute(0, 3, 1, 2).contiguous()
    if out is None:
        return res
    out.copy_(res)
    return out


def _softsplat_many(inputs, flow, metric, mode, outs=None, reuse_index=False, keep_quad=False):
    return [_softsplat(x, flow, metric, mode, None if outs is None else outs[k]) for k, x in enumerate(inputs)]


def _resize_bilinear_scale(x, size, src_scale, defect=False):
    (hi, wi), (ho, wo) = x.shape[2:], size

    def axis(n_in, n_out):
        mul = n_in / n_out if defect else src_scale
        s = (mul * (torch.arange(n_out, dtype=torch.float32) + 0.5) - 0.5).clamp(min=0)
        i0 = s.floor().clamp(max=n_in - 1)
        return i0.long(), (i0 + 1).clamp(max=n_in - 1).long(), s - i0

    y0, y1, ly = axis(hi, ho)
    x0, x1, lx = axis(wi, wo)
    out = torch.empty(x.shape[0], x.shape[1], ho, wo)
    for oy in range(ho):  # row by row: four taps, horizontal lerp first
        a, b, cc, d = x[:, :, y0[oy]][..., x0], x[:, :, y0[oy]][..., x1], x[:, :, y1[oy]][..., x0], x[:, :, y1[oy]][..., x1]
        out[:, :, oy] = (1 - ly[oy]) * ((1 - lx) * a + lx * b) + ly[oy] * ((1 - lx) * cc + lx * d)
    return out


def _to_inp(img_u8, dst_size):
    out = F.interpolate(img_u8.permute(2, 0, 1)[None].float() / 255.0, size=tuple(dst_size), mode="bilinear", align_corners=False)
    x4 = torch.zeros(dst_size[0], dst_size[1], 4)
    x4[..., :3] = out[0].permute(1, 2, 0)
    out._drba_x4 = (x4, out._version)
    return out


# ---- the IFNet stage glue, tap by tap: lerp_src per axis, 2 x 2 gathers at clamped coordinates, the running flow term by term
def _axis(n_in, n_out, mul, ac=False):
    """source index pair and the weight of the second tap of every output index along one axis (align_corners=False; ac: planted)"""
    i = torch.arange(n_out, dtype=torch.float32)
    s = i * ((n_in - 1) / max(n_out - 1, 1)) if ac else (mul * (i + 0.5) - 0.5).clamp(min=0)
    i0 = s.floor().clamp(max=n_in - 1)
    return i0.long(), (i0 + 1).clamp(max=n_in - 1).long(), s - i0


def _lerp_resize(x, size, mul, ac=False, tile_clamp=False):
    if mul == 1.0 and tuple(size) == tuple(x.shape[2:]) and not ac:
        return x  # weights (1, 0): the zero-weight taps are skipped
    y0, y1, ly = _axis(x.shape[2], size[0], mul, ac)
    x0, x1, lx = _axis(x.shape[3], size[1], mul, ac)
    if tile_clamp:  # planted: the footprint under a 32-pixel tile staged 17 columns wide instead of 18
        x1 = torch.minimum(x1, x0[(torch.arange(size[1]) // 32) * 32] + 16)
    ly = ly.view(-1, 1)
    r0, r1 = x[:, :, y0], x[:, :, y1]
    top = (1 - lx) * r0[..., x0] + lx * r0[..., x1]
    bot = (1 - lx) * r1[..., x0] + lx * r1[..., x1]
    return (1 - ly) * top + ly * bot


def _up(t, s, **kw):
    return _lerp_resize(t, (int(t.shape[2] * s), int(t.shape[3] * s)), 1.0 / s, **kw)


def _dn(x, s):
    return _lerp_resize(x, (int(x.shape[2] * (1.0 / s)), int(x.shape[3] * (1.0 / s))), float(s))


def _warp(x, flow, edge=False):
    n, _, h, w = x.shape
    gx = torch.linspace(-1.0, 1.0, w).view(1, 1, w) + flow[:, 0] / ((w - 1.0) / 2.0)
    gy = torch.linspace(-1.0, 1.0, h).view(1, h, 1) + flow[:, 1] / ((h - 1.0) / 2.0)
    return _bilinear(x, (gx + 1) * ((w - 1.0) / 2.0), (gy + 1) * ((h - 1.0) / 2.0), "border", edge)


def _rgbx(img):
    c = getattr(img, "_drba_x4", None)
    if c is None or c[1] != img._version:
        img._drba_x4 = (torch.stack([img[0, 0], img[0, 1], img[0, 2], torch.zeros_like(img[0, 0])], -1), img._version)
    return img._drba_x4[0]


def _frame(img, x4):
    """the frame as the gather reads it: from its [H, W, 4] copy where it carries a current one and the entry point takes it"""
    c = getattr(img, "_drba_x4", None)
    if x4 and c is not None and c[1] == img._version:
        return c[0][..., :3].permute(2, 0, 1)[None]
    return img


def _planar(f, as_planar=False):
    """features [1, 16, H, W] of either layout (as_planar, planted: the pair-only tensor [8, H, W, 2] read as planes)"""
    if not (f.dim() == 4 and f.shape[0] == 8 and f.shape[3] == 2):
        return f
    c2, h, w, _ = f.shape
    return f.reshape(1, 2 * c2, h, w) if as_planar else f.permute(0, 3, 1, 2).reshape(1, 2 * c2, h, w)


def _flow_update(tmp, flow_in, s):
    fd = _up(tmp[:, :4], s) * s
    return fd if flow_in is None else flow_in + fd


def _terms_flow(terms, tmp, s_last, defect=None):
    """the running flow: oldest term first, every product and sum in fp32, the newest head output last"""
    seq = list(terms) + [(tmp, s_last)]
    fl = None
    for k, (t, s) in enumerate(seq):
        last = k == len(seq) - 1
        d = _up(t[:, :4], s, tile_clamp=defect == "tile_clamp" and not last)
        if defect == "neighbour" and last:  # the pixel to the right
            d = d[..., torch.arange(1, d.shape[3] + 1).clamp(max=d.shape[3] - 1)]
        d = d * (s_last if defect == "oldest_scale" and k == 0 and not last else s)
        fl = d if fl is None else fl + d
    return fl


def _stage_core(img0, img1, f0, f1, timestep, flow, tmp_prev, sp, s, x4, defect=None):
    i0, i1 = _frame(img0, x4), _frame(img1, x4)
    f0, f1 = _planar(f0, defect == "pair_as_planar"), _planar(f1, defect == "pair_as_planar")
    tm = timestep if torch.is_tensor(timestep) else torch.full_like(i0[:, :1], float(timestep))
    if flow is None:
        return _dn(torch.cat((i0, i1, f0, f1, tm), 1), s)
    edge = defect == "edge_tap"
    x = torch.cat((_warp(i0, flow[:, :2], edge), _warp(i1, flow[:, 2:4], edge), _warp(f0, flow[:, :2], edge), _warp(f1, flow[:, 2:4], edge), tm,
                   _up(tmp_prev[:, 4:13], sp)), 1)
    fl = _dn(flow, s)
    return torch.cat((_dn(x, s), fl if defect == "flow_unscaled" else fl / s), 1)


def _ifblock_input(img0, img1, f0, f1, timestep, flow, tmp_prev, prev_scale, scale, out=None, defect=None):
    return _stage_core(img0, img1, f0, f1, timestep, flow, tmp_prev, prev_scale, scale, False, defect)


def _ifblock_input_lds(img0, img1, f0, f1, timestep, flow, tmp_prev, prev_scale, scale, out=None, fold=False, defect=None):
    if fold:
        flow = _flow_update(tmp_prev, flow, prev_scale)
    r = _stage_core(img0, img1, f0, f1, timestep, flow, tmp_prev, prev_scale, scale, False, defect)
    return (r, flow) if fold else r


def _stage_inputs(items, flows, tmp_prev, prev_scale, scale, out, fold=False, lds=True, terms=None, defect=None):
    folded = []
    for k, it in enumerate(items):
        tp = None if tmp_prev is None else tmp_prev[k:k + 1]
        if terms is not None:
            fl = _terms_flow([(t[k:k + 1], s) for t, s in terms], tp, prev_scale, defect)
        else:
            fl = None if flows is None else flows[k]
            if fold:
                fl = _flow_update(tp, fl, prev_scale)
                folded.append(fl)
        out[k:k + 1] = _stage_core(it[0], it[1], it[3], it[4], it[2], fl, tp, prev_scale, scale, lds and scale <= 2, defect)
    return folded if fold else None


_CONV_MEMO = {}  # the stand-in's result per (layer tensors, operands, epilogue, defect): an id picks no kernel here, 38 ids share one evaluation


def _refuse():
    from drba_amd import _lib
    raise _lib.DrbaHipError("drba_conv3x3 failed: unsupported (-2)")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class _Conv3x3:
    """ops.Conv3x3 in torch fp32: the same constructor and call.  `cfg` picks no kernel, but the one documented refusal is kept: the
    library's host-side table functions say which ids are the LDS-DMA members, and those refuse W % 4 != 0.  `defect` names the
    planted one-line variant (None: none)."""
    ACTS = {None: 0, False: 0, "none": 0, True: 1, "lrelu": 1, "prelu": 2, "relu": 3, "tanh10": 4}
    defect = None

    def __init__(self, weight, bias, stride=1, act=True, beta=None, device=None, cfg=None, pre_slope=None, post_slope=0.0):
        self.w, self.b, self.bias, self.cout, self.cin = weight, bias, bias, weight.shape[0], weight.shape[1]
        self.stride, self.act, self.beta, self.cfg, self.pre_slope, self.post_slope = stride, self.ACTS[act], beta, cfg, pre_slope, post_slope

    def _value(self, x, residual, residual2):
        d = self.defect
        xin = x if self.pre_slope is None else torch.where(x > 0, x, x * self.pre_slope)
        b = self.b
        if d == "bias_from_32" and b is not None:
            b = b.clone()
            b[32:] = 0.0
        y = F.conv2d(xin, self.w, b, stride=self.stride, padding=1)
        if d == "pre_on_residual" and residual is x:
            residual = xin
        if d == "res2_dropped":
            residual2 = None
        if self.beta is not None:
            bt = self.beta.reshape(1, -1, 1, 1)
            y = (y + residual) * bt if d == "beta_order" else y * bt + residual
        else:
            if residual is not None:
                y = y + residual
            if residual2 is not None:
                y = y + residual2
        if self.act == 1:
            return torch.where(y > 0, y, 0.2 * y)
        if self.act == 2:
            return torch.where(y > 0, y, (0.2 if d == "post_slope_02" else self.post_slope) * y)
        if self.act == 3:
            zero = torch.zeros_like(y)
            return torch.where(y > 0, y, zero) if d == "relu_swallows_nan" else torch.where(y > 0, y, torch.where(y != y, y, zero))
        return torch.tanh(y) * 10.0 if self.act == 4 else y

    def __call__(self, x, residual=None, out=None, residual2=None):
        if self.cfg is not None and x.shape[3] % 4 and op_checks.conv_id_class(op_checks.conv_lib(), self.cfg) == "dma":
            _refuse()
        key = (_ptr(self.w), _ptr(self.b), _ptr(self.beta), _ptr(x), _ptr(residual), _ptr(residual2), residual is x, self.stride, self.act,
               self.pre_slope, self.post_slope, self.defect)
        if key not in _CONV_MEMO:
            _CONV_MEMO[key] = (self._value(x, residual, residual2), x, residual, residual2)  # (the operands kept alive: their addresses are the key)
        y = _CONV_MEMO[key][0]
        if out is None:
            return y.clone()
        out.copy_(y)
        end = out.storage_offset() + out.numel()
        if self.defect == "store_past" and end < out.untyped_storage().nbytes() // 4:  # one element past the last output plane
            out.as_strided((1,), (1,), end).fill_(0.0)
        return out


def _conv_defect(name):
    return type(f"_Conv3x3_{name}", (_Conv3x3,), {"defect": name})


class _Deconv4x4:
    def __init__(self, weight, bias, pixel_shuffle=False, device=None, cfg=None, pre_slope=None):
        self.w, self.b, self.ps, self.pre_slope = weight, bias, pixel_shuffle, pre_slope

    def __call__(self, x, out=None):
        xin = x if self.pre_slope is None else torch.where(x > 0, x, x * self.pre_slope)
        y = F.conv_transpose2d(xin, self.w, self.b, stride=2, padding=1)
        y = STANDIN["pixel_shuffle2"](y) if self.ps else y
        return y if out is None else out.copy_(y)


def _conv3x3_shuffle(layer, x):
    return STANDIN["pixel_shuffle2"](layer(x))


def _conv3x3_shuffle_launch(layer, x, out, cfg):
    """drba_conv3x3_shuffle's return code; every family-4 stride-1 id is taken to carry the store form"""
    out.copy_(_conv3x3_shuffle(layer, x))
    return 0


def _stage_conv0_ok(conv, H, W, scale, prev_scale, items=None):
    if scale == 2:
        return prev_scale == 4 and conv.cout in (16, 32) and items is not None and all(_frame(it[0], True) is not it[0] for it in items)
    return scale == 1 and prev_scale == 2 and conv.cout == 16


def _stage_conv0(items, flows, tmp_prev, prev_scale, conv, fold=False, terms=None, scale=1, out=None):
    h, w = items[0][0].shape[2:]
    xin = torch.empty(len(items), 52, h // scale, w // scale)
    fo = _stage_inputs(items, flows, tmp_prev, prev_scale, scale, xin, fold=fold, terms=terms)
    return F.leaky_relu(F.conv2d(xin, conv.w, conv.b, stride=2, padding=1), 0.2), fo


def _ifblock_update(tmp, flow_in, H, W, scale, want_mask_feat=False):
    flow = _flow_update(tmp, flow_in, scale)
    return (flow, _up(tmp[:, 4:5], scale), _up(tmp[:, 5:13], scale)) if want_mask_feat else flow


def _flow_updates(tmp, flows, H, W, scale, whole=False, defect=False):
    return [_flow_update(tmp[k:k + 1], flows[0 if defect else k], scale) for k in range(tmp.shape[0])]


def _blend(i0, i1, flow, logit):
    m = 1.0 / (1.0 + torch.exp(-logit))
    return _warp(i0, flow[:, :2]) * m + _warp(i1, flow[:, 2:4]) * (1.0 - m)


def _warp_blend(img0, img1, flow, tmp_last, scale, defect=False):
    return _blend(img0, img1, flow, _up(tmp_last[:, 4:5], scale, ac=defect))


def _warp_blend_fold(img0, img1, flow_prev, tmp_last, scale):
    return _blend(img0, img1, _flow_update(tmp_last, flow_prev, scale), _up(tmp_last[:, 4:5], scale))


def _warp_blend_lazy(items, terms, tmp_last, scale, defect=None):
    return [_blend(_frame(it[0], True), _frame(it[1], True), _terms_flow([(t[k:k + 1], s) for t, s in terms], tmp_last[k:k + 1], scale, defect),
                   _up(tmp_last[k:k + 1, 4:5], scale)) for k, it in enumerate(items)]


# ---- the GMFlow transformer kernels: attention window by window with an explicit roll index map and region ids, both attentions
# as a running (max, sum, weighted sum) over 64-key chunks, the linear layer with its epilogues written out
def _flash(Q, K, vals, scale, L, bias=None, tail_keys=False, no_rescale=False):
    """softmax(Q K^T / scale + bias) vals over chunks of 64 keys, the last chunk padded with copies of key L - 1 that take no part"""
    n = Q.shape[0]
    m, l, acc = torch.full((n,), float("-inf")), torch.zeros(n), torch.zeros(n, vals.shape[1])
    for c0 in range(0, L, 64):
        pos = c0 + torch.arange(64)
        idx = pos.clamp(max=L - 1)
        s = (Q @ K[idx].t()) / scale
        if bias is not None:
            s = s + bias[:, idx]
        if not tail_keys:
            s[:, pos >= L] = float("-inf")
        m_new = torch.maximum(m, s.max(1).values)
        ref = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)  # (a chunk that is masked out altogether: planted -inf mask only)
        alpha = torch.ones(n) if no_rescale else torch.exp(m - ref)
        p = torch.exp(s - ref[:, None])
        l, acc, m = l * alpha + p.sum(1), acc * alpha[:, None] + p @ vals[idx], m_new
    return acc / l[:, None]


def _window_attention(q, k, v, h, w, splits, shift, scale, terms=None, defect=None):
    b, n, c = q.shape
    wh, ww = h // splits, w // splits
    sh, sw = (wh // 2, ww // 2) if shift else (0, 0)
    L = wh * ww
    t = torch.arange(L)
    ly, lx = t // ww, t % ww
    out = torch.zeros(b, n, c)
    for win in range(b * splits * splits):
        bi, wi = divmod(win, splits * splits)
        y, x = (wi // splits) * wh + ly, (wi % splits) * ww + lx  # position in the rolled image
        rows, bias = ((y + sh) % h) * w + (x + sw) % w, None    # the row it came from
        if shift:
            second = h - wh if defect == "region_bound" else h - sh
            region = 3 * ((y >= h - wh).long() + (y >= second).long()) + (x >= w - ww).long() + (x >= w - sw).long()
            bias = torch.where(region[:, None] != region[None, :], float("-inf") if defect == "mask_inf" else -100.0, 0.0)
        src = 0 if defect == "no_batch" else bi
        res = _flash(q[src, rows], k[src, rows], v[src, rows], scale, L, bias, defect == "tail_keys", defect == "no_rescale")
        out[bi, (y * w + x) if defect == "unrolled_out" else rows] = res
    return out


def _global_expect2(q_tok, k_tok, vals, w, scale, defect=None):
    L = q_tok.shape[0]
    key = torch.arange(L)
    cx, cy = (key % w).float(), (key // w).float()
    v2 = torch.stack((cy, cx) if defect == "xy_exchanged" else (cx, cy), 1) if vals is None else vals.t()
    out = _flash(q_tok, k_tok, v2, scale, L).t()
    if vals is None and defect != "own_coordinate":
        out = out - torch.stack((cx, cy))
    return out.contiguous()


class _LinearSplit:
    """ops.LinearSplit in torch fp32: y = x w^T as a sum over 32-feature chunks, + bias, then the epilogue written out"""
    defect = None

    def __init__(self, weight, bias=None, gelu=False, device=None, terms=None):
        self.w, self.b, self.gelu = weight, bias, gelu
        self.n, self.k = weight.shape

    def _gemm(self, x):
        y = torch.zeros(x.shape[0], self.n)
        for c0 in range(0, self.k, 32):
            y += x[:, c0:c0 + 32] @ self.w[:, c0:c0 + 32].t()
        if self.b is not None:
            b = self.b.clone()
            if self.defect == "bias_to_128":
                b[128:] = 0.0
            y = y + b
        return y

    def __call__(self, x):
        y = self._gemm(x.reshape(-1, self.k))
        if self.gelu:
            if self.defect == "tanh_gelu":
                y = 0.5 * y * (1 + torch.tanh(0.7978845608028654 * (y + 0.044715 * y ** 3)))
            else:
                y = 0.5 * y * (1 + torch.erf(y * 0.7071067811865476))
        return y.view(*x.shape[:-1], self.n)

    def cat(self, x1, x2):
        x = torch.cat((x1, x2), -1)
        if self.defect == "cat_split":  # the chunk behind the split still read from x1's side
            k1 = x1.shape[-1]
            x[..., k1:k1 + 32] = x[..., k1 - 32:k1]
        return self(x)

    def layernorm(self, x, ln_w, ln_b, residual=None, eps=1e-5):
        y = self._gemm(x.reshape(-1, self.k))
        mean = y.sum(1, keepdim=True) / 128
        if self.defect == "one_pass_variance":
            var = (y * y).sum(1, keepdim=True) / 128 - mean * mean
        else:
            var = ((y - mean) ** 2).sum(1, keepdim=True) / (127 if self.defect == "unbiased_variance" else 128)
        out = (y - mean) / torch.sqrt(var + eps) * ln_w + ln_b
        return out if residual is None else residual + out


def _lin_defect(name):
    return type(f"_LinearSplit_{name}", (_LinearSplit,), {"defect": name})


# ---- IFNet's encoder as one call: the four layers in fp32, both layouts from the same values
def _head_layers(x, layers):
    c0, c1, c2, c3 = layers
    y = F.leaky_relu(F.conv2d(x, c0.w, c0.b, stride=2, padding=1), 0.2)
    y = F.leaky_relu(F.conv2d(y, c1.w, c1.b, padding=1), 0.2)
    y = F.leaky_relu(F.conv2d(y, c2.w, c2.b, padding=1), 0.2)
    return F.conv_transpose2d(y, c3.w, c3.b, stride=2, padding=1)


def _head_fused(img, layers, holder, planar=True, defect=None):
    n, c, h, w = img.shape
    if n != 1 or c != 3 or h % 2 or w % 4:
        return None
    if defect == "ring_not_zero":  # the positions outside the map hold what the layers make of zeros, not zero
        f = _head_layers(F.pad(img, (8, 8, 8, 8)), layers)[:, :, 8:-8, 8:-8].contiguous()
    elif defect == "window_one_short":  # every 16 x 64 tile from a frame window with a halo of 6 pixels where 7 are read
        f = torch.empty(1, 16, h, w)
        for y0 in range(0, h, 16):
            for x0 in range(0, w, 64):
                ya, xa = max(y0 - 6, 0), max(x0 - 6, 0)
                t = _head_layers(img[:, :, ya:min(y0 + 22, h), xa:min(x0 + 70, w)], layers)
                f[:, :, y0:y0 + 16, x0:x0 + 64] = t[:, :, y0 - ya:y0 - ya + 16, x0 - xa:x0 - xa + 64]
    else:
        f = _head_layers(img, layers)
    fp = torch.stack([f[0, 0::2], f[0, 1::2]], -1).contiguous()
    if defect == "pair_swapped":
        fp = fp.flip(-1).contiguous()
    if defect == "tail_unwritten" and w % 8 == 4:  # the planar tail store of a last half tile: the buffer is left as allocated
        f[..., w - 4:] = float("nan")
    if not planar:
        fp._drba_is_pair = True
        return fp
    f._drba_pair = fp
    return f


def _is_pair(f):
    return bool(getattr(f, "_drba_is_pair", False)) or bool(f.dim() == 4 and f.shape[0] == 8 and f.shape[3] == 2 and f.shape[1] > 2 and f.shape[2] > 2)


def _features_planar(f):
    if not _is_pair(f):
        return f
    c2, h, w, _ = f.shape
    return f.permute(0, 3, 1, 2).reshape(1, 2 * c2, h, w).contiguous()


class _RifeSplats:
    """The fused RIFE splats in the kernels' form: a reach per source tile as the pre-pass rounds it, a halo variant per output tile
    from the 3 x 3 reach entries around it (16 everywhere when the launch has more tiles than the reach map has words), and every
    (source, corner) pair added once -- a short source by the tile that owns the corner, if the source lies in that tile's window;
    a long one by the pre-pass, which also leaves a flag for the tile.  A tile holds kCAP records in key order; the rest go through the
    accumulator, corner by corner of that tile.  The workspace is the zeroed buffer the entry points share: reach words in front,
    everything behind them zero again on return.  `defect`: one rule of the above changed (RIFE_DEFECTS below)."""

    def __init__(self, defect=None, reach_words=det_common.REACH_WORDS):
        self.defect, self.reach_words, self.det = defect, reach_words, False
        self.ws = torch.zeros(det_common.REACH_WORDS + (1 << 16))

    def namespace(self):
        return {k: getattr(self, k) for k in ("flow_reverse", "drm_rife_linear", "drm_rife_linear_many", "drm_rife_nonlinear",
                                              "drm_rife_nonlinear_many", "set_deterministic", "_zero_workspace")}

    def set_deterministic(self, on):
        was, self.det = self.det, bool(on)
        return was

    def _zero_workspace(self, device, nfloats):
        return self.ws

    def _slots(self, kx, ky, ok, item, src, n, h, w):
        """per corner (dy, dx): the slot of the source among the records of the corner's tile, in key order (-1: the corner is not the
        first of the source's footprint in that tile, or names no tile)"""
        ty_n, tx_n = det_common.tiles_of(h, w)
        keys, tiles, masks = [], [], []
        for dy in (0, 1):
            for dx in (0, 1):
                cx, cy = kx + dx, ky + dy
                first = ((dx == 0) | (cx % det_common.TX == 0)) & ((dy == 0) | (cy % det_common.TY == 0))
                m = ok & first & (cx >= 0) & (cy >= 0) & (cx // det_common.TX < tx_n) & (cy // det_common.TY < ty_n)
                tX, tY = cx // det_common.TX, cy // det_common.TY
                tile = (item * ty_n + tY) * tx_n + tX
                key = (ky - tY * det_common.TY + 1) * (det_common.TX + 1) + (kx - tX * det_common.TX + 1)
                keys.append(((tile * 600 + key) * (h * w) + src)[m])
                tiles.append(tile[m])
                masks.append(m)
        key, tile = torch.cat(keys), torch.cat(tiles)
        order = torch.argsort(key)
        ts = tile[order]
        pos = torch.arange(ts.numel())
        new = torch.ones_like(ts, dtype=torch.bool)
        new[1:] = ts[1:] != ts[:-1]
        start = torch.cummax(torch.where(new, pos, torch.zeros_like(pos)), 0).values
        rank = torch.empty_like(pos)
        rank[order] = pos - start
        out, at = [], 0
        for m in masks:
            s = torch.full((n, h, w), -1, dtype=torch.long)
            k = int(m.sum())
            s[m] = rank[at:at + k]
            at += k
            out.append(s)
        return out  # index 2 * dy + dx

    def _splat(self, flow, val, fill, mode0):
        d, TX, TY = self.defect, det_common.TX, det_common.TY
        n, _, h, w = flow.shape
        nv = val.shape[1]
        ty_n, tx_n = det_common.tiles_of(h, w)
        finite, short = det_common.source_class(flow)
        reach = det_common.tile_reach(flow, tight=1 if d == "reach_tight" else 2 if d == "reach_too_tight" else 0)
        if d == "item0_reach":
            reach = reach[0:1].expand(n, ty_n, tx_n)
        if n * ty_n * tx_n <= self.reach_words:
            self.ws[:n * ty_n * tx_n] = reach.flatten().float()
            nb = reach if d == "own_reach_only" else F.max_pool2d(reach[:, None].float(), 3, 1, 1)[:, 0].long()
            variant = torch.where(nb <= 4, 4, torch.where(nb <= 8, 8, 16))
        else:
            variant = torch.full((n, ty_n, tx_n), 4 if d == "no_map_as_r4" else 16)
        xs, ys = _grid(n, h, w)
        X = torch.where(finite, xs + flow[:, 0], torch.zeros_like(xs))
        Y = torch.where(finite, ys + flow[:, 1], torch.zeros_like(ys))
        fx, fy = X.floor(), Y.floor()
        kx, ky = fx.clamp(-1e9, 1e9).long(), fy.clamp(-1e9, 1e9).long()
        xi, yi = xs.long(), ys.long()
        item = torch.arange(n).view(n, 1, 1).expand(n, h, w)
        src = yi * w + xi
        slots = None
        if d in ("spill_dropped", "spill_all_corners") and int(det_common.tile_record_totals(flow).max()) > det_common.CAP:
            slots = self._slots(kx, ky, finite & short, item, src, n, h, w)
        vals = torch.cat([val, torch.ones_like(val[:, :1])], 1).permute(0, 2, 3, 1)
        acc = torch.zeros(n * h * w, nv + 1)
        corner, long_landed = {}, False
        for dy in (0, 1):
            for dx in (0, 1):
                px, py = kx + dx, ky + dy
                wgt = (X - fx if dx else (fx + 1) - X) * (Y - fy if dy else (fy + 1) - Y)
                inmap = finite & (px >= 0) & (px < w) & (py >= 0) & (py < h)
                tX, tY = (px // TX).clamp(0, tx_n - 1), (py // TY).clamp(0, ty_n - 1)
                R = variant[item, tY, tX]
                x0, y0 = tX * TX, tY * TY
                far = 1 if d == "window_one_short" else 0
                inwin = (xi >= x0 - R) & (xi <= x0 + TX + R - 1 - far) & (yi >= y0 - R) & (yi <= y0 + TY + R - 1 - far)
                keep = inmap & (~short | inwin)
                long_landed = long_landed or bool((inmap & ~short).any())
                corner[(dy, dx)] = (px, py, wgt, inmap, (item * ty_n + tY) * tx_n + tX)
                if slots is not None:
                    fdx = torch.where(px % TX == 0, dx, 0) if dx else torch.zeros_like(px)  # the first corner of the footprint in this tile
                    fdy = torch.where(py % TY == 0, dy, 0) if dy else torch.zeros_like(py)
                    slot = torch.stack(slots)[2 * fdy + fdx, item, yi, xi]
                    if d == "spill_dropped":
                        keep = keep & ~(short & (slot >= det_common.CAP))
                acc.index_add_(0, (item * h * w + py * w + px)[keep], vals[keep] * wgt[keep].unsqueeze(1))
        if slots is not None and d == "spill_all_corners":
            for c, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                spilled = slots[c] >= det_common.CAP  # the source is a spilled record of the tile of this corner
                for px, py, wgt, inmap, tile in corner.values():
                    extra = spilled & inmap & (tile != corner[(dy, dx)][4])
                    acc.index_add_(0, (item * h * w + py * w + px)[extra], vals[extra] * wgt[extra].unsqueeze(1))
        if d == "stale_dirty" and long_landed:
            self.ws[det_common.REACH_WORDS + 17] = 1e-45  # a flag of the pre-pass nobody cleared
        acc = acc.view(n, h, w, nv + 1).permute(0, 3, 1, 2)
        sw = acc[:, nv:]
        nrm = sw + 0.0000001
        gap = (sw / nrm) < 0.999
        if mode0:
            return torch.where(gap, torch.full_like(flow, float(max(h, w))), -1.0 * (acc[:, :nv] / nrm)) * 2.0
        return torch.where(gap, fill, acc[:, :nv] / nrm).contiguous()

    def flow_reverse(self, flow):
        return self._splat(flow, flow, None, True)

    def drm_rife_linear(self, a, b, t, eps=1e-4, t_dev=None):
        u = _drm_ratio(a, b, eps)[1] * (float(t_dev[0]) if t_dev is not None else t) * 2
        return self._splat(a * u, u, u, False)

    def drm_rife_nonlinear(self, a, b, t, eps=1e-4, precision=1e-3):
        u = odrm.drm_to_t(_drm_ratio(a, b, eps)[1], t, precision)
        return self._splat(a * u, u, u, False)

    def _many(self, jobs, fn):
        """(one launch: the jobs are the items of one reach map)"""
        a, b = torch.cat([j[0] for j in jobs]), torch.cat([j[1] for j in jobs])
        us = torch.cat([fn(j[0], j[1], j[2]) for j in jobs])
        out = self._splat(a * us, us, us, False)
        return [out[k:k + 1] for k in range(len(jobs))]

    def drm_rife_linear_many(self, jobs, eps=1e-4):
        return self._many(jobs, lambda a, b, t: _drm_ratio(a, b, eps)[1] * t * 2)

    def drm_rife_nonlinear_many(self, jobs, eps=1e-4, precision=1e-3):
        return self._many(jobs, lambda a, b, t: odrm.drm_to_t(_drm_ratio(a, b, eps)[1], t, precision))


STANDIN = dict(
    _RifeSplats().namespace(),
    head_fused=_head_fused, is_pair=_is_pair, features_planar=_features_planar,
    window_attention=_window_attention, global_expect2=_global_expect2, LinearSplit=_LinearSplit,
    softmax_rows_=_softmax_rows_, instance_norm=_instance_norm, conv_direct=_conv_direct, local_corr_flow=_local_corr_flow,
    local_attn_flow=_local_attn_flow, convex_upsample=_convex_upsample, flow_warp=_flow_warp, backwarp=_backwarp,
    resize_bilinear_ac=_resize_bilinear_ac, layernorm=_layernorm, timestep_fix=_timestep_fix, drm_ratio=_drm_ratio,
    metric_input=_metric_input, to_inp=_to_inp, softsplat=_softsplat, softsplat_many=_softsplat_many,
    resize_bilinear_scale=_resize_bilinear_scale, flow_distance=lambda f: (f[:, 0:1] * f[:, 0:1] + f[:, 1:2] * f[:, 1:2]).sqrt(),
    gelu=lambda x: 0.5 * x * (1 + torch.erf(x * 0.7071067811865476)),
    bmm=lambda a, b, trans_b: torch.einsum("bmk,bnk->bmn", a, b) if trans_b else torch.einsum("bmk,bkn->bmn", a, b),
    add_act=lambda a, b, relu=False: (a + b).clamp(min=0) if relu else a + b,
    affine=lambda a, mul, add: a * mul + add,
    channel_normalize3=lambda x, mean, std: (x - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1),
    mul_map=lambda x, m: x * m,
    clamp=lambda x, lo, hi: torch.where(x != x, x, torch.minimum(torch.maximum(x, torch.tensor(lo)), torch.tensor(hi))),
    pixel_shuffle2=lambda x: torch.stack([x[:, i::4] for i in range(4)], 2).view(x.shape[0], x.shape[1] // 4, 2, 2, *x.shape[2:])
    .permute(0, 1, 4, 2, 5, 3).reshape(x.shape[0], x.shape[1] // 4, 2 * x.shape[2], 2 * x.shape[3]),
    pair_interleaved=lambda f: torch.stack([f[0, 0::2], f[0, 1::2]], -1),
    quad_interleaved=lambda x: torch.stack([x[:, i::4].flatten(2) for i in range(4)], -1),
    rgbx=_rgbx, ifblock_input=_ifblock_input, ifblock_input_lds=_ifblock_input_lds, stage_inputs=_stage_inputs, Conv3x3=_Conv3x3,
    stage_conv0_ok=_stage_conv0_ok, stage_conv0=_stage_conv0, ifblock_update=_ifblock_update, flow_updates=_flow_updates,
    warp_blend=_warp_blend, warp_blend_fold=_warp_blend_fold, warp_blend_lazy=_warp_blend_lazy,
    fill_holes=lambda aligned, cover, value: torch.where(cover < 0.999, value, aligned),
    drm_retime=lambda d, t, precision=1e-3: odrm.drm_to_t(d, t, precision),
    Deconv4x4=_Deconv4x4, conv3x3_shuffle=_conv3x3_shuffle, conv3x3_shuffle_launch=_conv3x3_shuffle_launch,
)


class Recorder:
    """The stand-in namespace; remembers which operators a check asked for."""

    def __init__(self, **override):
        self.fns, self.used = dict(STANDIN, **override), set()

    def __getattr__(self, name):
        if name not in self.fns:
            raise AttributeError(name)
        self.used.add(name)
        return self.fns[name]


def _passes(row):
    return bool(row[1] <= row[2])  # the pass test of every parity row (_assert_rows, report.record)


@pytest.fixture(scope="module")
def clean():
    """{section: (rows, operators the check called)} of the stand-in without a defect"""
    out = {}
    for title, check in op_checks.CHECKS:
        ns = Recorder()
        with torch.no_grad():
            out[title] = (check(CPU, ns), set(ns.used))
    return out


# ----------------------------------------------------------------------------------------- 1. the references
# What an fp32 evaluation may differ from the fp64 reference by, from the number format and the conditioning alone.  Default:
# the rule's own first term, 2e-5 * max(1, |ref|max) (a few hundred ulps of the largest value: sums of up to ~1e3 rounded terms).
# Ill-conditioned rows, by name:
FLOOR_BOUNDS = (
    # (x - mean) / sqrt(var + eps) with |mean| = 1e3, var = 1e-4: rounding the mean (or x - mean) to fp32 moves the numerator by
    # up to 2^-24 * 1e3 = 6e-5, i.e. the output by 6e-5 / sqrt(1.1e-4) = 5.7e-3; two such roundings (sum, mean)
    ("instance_norm", "mean 1e3", 2 * EPS32 * 1e3 / (1e-4 + 1e-5) ** 0.5),
    # a constant plane 3.7: the fp32 mean of 1961 equal values is off by a few ulps (4 * 2^-24 * 3.7), over sqrt(eps)
    ("instance_norm", "constant plane", 16 * EPS32 * 3.7 / 1e-5 ** 0.5),
    # exp(s - max) with |s| up to ~4 * 80: the fp32 score difference carries 2^-24 * 640 relative error into every term
    ("softmax_rows_", "|scores|~80", 4 * EPS32 * 640),
    # LayerNorm of 100 +- 0.1: the pre-norm value rounds to fp32 with 2^-24 * 128 (the binade of 100), the mean likewise; over a
    # deviation of 0.1, times a gain of up to 2
    ("linear_split", "mean 100 deviation 0.1", 2 * EPS32 * 128 / 0.1 * 2),
)


def _floor_bound(row):
    for op, key, bound in FLOOR_BOUNDS:
        if row.op == op and key in row[0]:
            return bound
    base = 2e-5 * max(1.0, row.refmax)
    if row.op == "window_attention":
        # a score is a sum of 128 products, off by a few 2^-24 |score|max in fp32 (more where the scale is folded into q first); exp
        # carries that absolute error of its argument into every probability as a relative one, twice (numerator, normaliser)
        return base + 16 * EPS32 * row.smax * max(1.0, row.refmax)
    return base


def _row_tol(row):
    """the tolerance a row's rule gives, from what the row records: the one rule of the series, or one of the three bars the
    transformer rows keep (tests/op_checks.py attn_row, gcorr_rows, lin_row)"""
    rule = getattr(row, "tol_rule", None)
    if rule == "two-term":
        return max(op_checks.rule_tol(row.refmax, row.floor), 3.0 * row.fmt_floor)
    if rule == "coords":
        return max(2e-5, 3.0 * row.floor) * max(1.0, row.w / 16.0)
    if rule == "linear":
        assert row.bar in (5e-6, 1e-5)
        return row.bar * max(1.0, row.refmax)
    assert rule is None
    return op_checks.rule_tol(row.refmax, row.floor)


def test_fp64_references_agree_with_the_fp32_forms(clean):
    n = 0
    for title, (rows, _) in clean.items():
        for row in rows:
            if row.floor is None:
                continue
            n += 1
            assert row.floor <= _floor_bound(row), f"{row[0]}: fp32 form vs fp64 reference {row.floor:.3e} > {_floor_bound(row):.3e}"
            assert row[2] == _row_tol(row)  # the one tolerance rule (or the named bar of a transformer row), nothing else
    assert n > 200


def test_references_where_aten_is_not_the_specification():
    """The two written-out cases of op_checks: zeros padding at a non-finite coordinate, InstanceNorm of one element."""
    x = torch.arange(24.0).view(1, 2, 3, 4)
    flow = torch.zeros(1, 2, 3, 4)
    flow[0, 0, 1, 1], flow[0, 1, 2, 2] = float("inf"), float("-inf")
    for ref in (op_checks.flow_warp_ref(x, flow), op_checks.backwarp_ref(x, flow, "zeros")):
        assert float(ref[0, :, 1, 1].abs().max()) == 0.0 and float(ref[0, :, 2, 2].abs().max()) == 0.0
        keep = torch.ones(3, 4, dtype=torch.bool)
        keep[1, 1] = keep[2, 2] = False
        assert torch.allclose(ref[0][:, keep], x[0][:, keep], atol=1e-5)  # zero flow elsewhere: the identity
    border = op_checks.backwarp_ref(x, flow, "border")  # border padding clamps the coordinate: a finite answer, from ATen
    assert torch.allclose(border[0, :, 1, 1], x[0, :, 1, 3], atol=1e-5) and torch.allclose(border[0, :, 2, 2], x[0, :, 0, 2], atol=1e-5)
    assert torch.equal(op_checks._inorm_ref(torch.full((2, 3, 1, 1), 5.0), False), torch.zeros(2, 3, 1, 1))


# ----------------------------------------------------------------------------------------- 2. the stand-in passes
def test_standin_passes_every_check(clean):
    bad = [r for rows, _ in clean.values() for r in rows if not _passes(r)]
    assert not bad, "\n".join(f"{r[0]}: err={r[1]:.3e} tol={r[2]:.1e} {r[3]}" for r in bad)
    ops_seen = set().union(*(used for _, used in clean.values()))
    assert ops_seen == set(STANDIN), sorted(set(STANDIN) ^ ops_seen)  # every operator of the issue is exercised by some check
    # SPLAT_CHECKS (what the deterministic-mode tests split CHECKS by) is exactly the families that call the generic splat
    assert set(op_checks.SPLAT_CHECKS) == {check for title, check in op_checks.CHECKS if {"softsplat", "softsplat_many"} & clean[title][1]}


def test_metric_input_masks_are_mostly_stable_and_two_sided(clean):
    rows = clean["op metric_input"][0]
    shares = [r for r in rows if "unstable share" in r[0]]
    assert len(shares) == 6 and all(r[1] <= op_checks.UNSTABLE_CAP for r in shares)
    assert len([r for r in rows if "wrong stable decisions" in r[0]]) == 6


# ----------------------------------------------------------------------------------------- 3. planted defects
def _with(fn, defect=True):
    """fn with its planted defect: the only one it has, or the named one of several"""
    variant = lambda *a, **k: fn(*a, defect=defect, **k)  # noqa: E731
    variant.defect = defect
    return variant


DEFECTS = (  # (operator of the stand-in, its defective variant, the operator family that must fail, a row that must fail)
    ("softmax_rows_", _with(_softmax_rows_), "softmax_rows_", "masked"),
    ("instance_norm", _with(_instance_norm), "instance_norm", "1x5"),
    ("local_attn_flow", _with(_local_attn_flow), "local_attn_flow", "5x7"),
    ("convex_upsample", _with(_convex_upsample), "convex_upsample", "x4 5x7"),
    ("resize_bilinear_ac", _with(_resize_bilinear_ac), "resize_bilinear_ac", "18x30->36x60"),
    ("metric_input", _with(_metric_input), "metric_input", "wrong stable decisions"),
    ("timestep_fix", _with(_timestep_fix), "timestep_fix", "out0"),
    ("conv_direct", _with(_conv_direct), "conv_direct", "->17"),
    # beyond the issue's eight: the wrong hole test in fill_holes, an fp64-exact but differently rounded retiming walk, a
    # border clamp where zeros padding is meant, the -1e4 of out-of-image correlation taps forgotten
    ("fill_holes", lambda a, c, v: torch.where(c <= 0.999, v, a), "fill_holes", "fill_holes"),
    ("drm_retime", lambda d, t, precision=1e-3: _retime_regrouped(d, t, precision), "drm_retime", "t=0.2"),
    ("flow_warp", lambda x, f: _backwarp(x, f, "border"), "flow_warp", "amp30"),
    ("local_corr_flow", lambda a, b, r: _local_corr_flow(F.pad(a, (r, r, r, r)), F.pad(b, (r, r, r, r)), r)[:, :, r:-r, r:-r].contiguous(),
     "local_corr_flow", "13x45"),
    # the generic splat: the carry of scan_sums' second round, the key column / row of footprints that start at -1, the tail
    # of the 16-channel chunk, the per-image offset of the segment table, the eps variants; the resize's multiplier
    ("softsplat", _with(_softsplat, "lost_keys"), "softsplat", "1024x1280"),
    ("softsplat", _with(_softsplat, "no_minus1"), "softsplat", "borders"),
    ("softsplat", _with(_softsplat, "tail_repeats"), "softsplat", "N=2 C=17"),
    ("softsplat", _with(_softsplat, "base_of_image0"), "softsplat", "N=3 C=5"),
    ("softsplat", _with(_softsplat, "zeroeps_as_addeps"), "softsplat", "soft-zeroeps normaliser"),
    ("resize_bilinear_scale", _with(_resize_bilinear_scale), "resize_bilinear_scale", "37x53"),
    # the IFNet stage glue: the oldest term times the newest scale; term taps clamped at a tile-local footprint one column short;
    # the left tap of a sample in the last column; flow / scale forgotten; the mask upsampled with align_corners=True; the S1 blend
    # reading the last head's flow at the right-hand neighbour; item 0's prior flow for every item; pair-only features read as planes
    ("stage_inputs", _with(_stage_inputs, "oldest_scale"), "stage_inputs", "lazy 64x128 s=1 terms=(16, 8, 4) planar"),
    ("warp_blend_lazy", _with(_warp_blend_lazy, "tile_clamp"), "warp_blend_lazy", "38x66 last=1 terms=(2,)"),
    ("ifblock_input_lds", _with(_ifblock_input_lds, "edge_tap"), "ifblock_input_lds", "integer"),
    ("ifblock_input", _with(_ifblock_input, "flow_unscaled"), "ifblock_input", "s=8 smooth t=map flow"),
    ("warp_blend", _with(_warp_blend), "warp_blend", "head s=2"),
    ("warp_blend_lazy", _with(_warp_blend_lazy, "neighbour"), "warp_blend_lazy", "S1 48x80"),
    ("flow_updates", _with(_flow_updates), "flow_updates", "item 1"),
    ("ifblock_input", _with(_ifblock_input, "pair_as_planar"), "ifblock_input", "features=pair-only features"),
    # the convolution epilogue forms: residual2 dropped; (y + x) * beta for y * beta + x; post_slope read as LeakyReLU's 0.2; the
    # pre-activation applied to a residual that is the input; bias zeroed from output channel 32 on; one store one element past the
    # last output plane (the guard row's); a ReLU that answers 0 for a NaN
    ("Conv3x3", _conv_defect("res2_dropped"), "conv_forms", "pre+res+res2"),
    ("Conv3x3", _conv_defect("beta_order"), "conv_forms", "resconv res is in"),
    ("Conv3x3", _conv_defect("post_slope_02"), "conv_forms", "bias+prelu(0.1)"),
    ("Conv3x3", _conv_defect("pre_on_residual"), "conv_forms", "pre+res=in"),
    ("Conv3x3", _conv_defect("bias_from_32"), "conv_forms", "64->40"),
    ("Conv3x3", _conv_defect("store_past"), "conv_forms", "in front of and behind out"),
    ("Conv3x3", _conv_defect("relu_swallows_nan"), "conv_forms", "NaN, -inf"),
    # the transformer kernels.  Window attention: the region mask as -inf; the second row boundary of the region ids at h - wh
    # instead of h - sh (the exchange the other way round -- h - sh for the first boundary -- labels the same partition of every window
    # and is no defect); the padding keys of the last chunk left in; no rescale when the running maximum moves; the output row
    # written at the rolled position; every window read from image 0
    ("window_attention", _with(_window_attention, "mask_inf"), "window_attention", "amp3 scale1"),
    ("window_attention", _with(_window_attention, "region_bound"), "window_attention", "shift1"),
    ("window_attention", _with(_window_attention, "tail_keys"), "window_attention", "(L=65="),
    ("window_attention", _with(_window_attention, "no_rescale"), "window_attention", "late maximum"),
    ("window_attention", _with(_window_attention, "unrolled_out"), "window_attention", "shift1"),
    ("window_attention", _with(_window_attention, "no_batch"), "window_attention", "b2 "),
    # the global expectation: the query's own coordinate left in; x and y of the key coordinates exchanged
    ("global_expect2", _with(_global_expect2, "own_coordinate"), "global_expect2", "coords 5x31"),
    ("global_expect2", _with(_global_expect2, "xy_exchanged"), "global_expect2", "coords 31x5"),
    # the linear layer: the tanh approximation for the erf GELU; the LayerNorm's variance over 127, and as E x^2 - mean^2; the split
    # of the concatenated input one chunk late; no bias past the first 128-feature tile
    ("LinearSplit", _lin_defect("tanh_gelu"), "linear_split", "gelu=1"),
    ("LinearSplit", _lin_defect("unbiased_variance"), "linear_split", "+ LayerNorm [70x64] bias=1"),
    ("LinearSplit", _lin_defect("one_pass_variance"), "linear_split", "mean 100 deviation 0.1"),
    ("LinearSplit", _lin_defect("cat_split"), "linear_split", "cat K1=32 K2=32"),
    ("LinearSplit", _lin_defect("bias_to_128"), "linear_split", "-> 129 gelu=0 bias=1"),
    # the fused encoder: the out-of-map rings of the intermediates not zeroed; the frame window one pixel short of the 7 a tile reads
    # beyond its edge; the last four planar columns of a W % 8 == 4 frame not stored; the two channels of a pair exchanged
    ("head_fused", _with(_head_fused, "ring_not_zero"), "head_fused", "zero frame 18x68"),
    ("head_fused", _with(_head_fused, "window_one_short"), "head_fused", "38x140"),
    ("head_fused", _with(_head_fused, "tail_unwritten"), "head_fused", "18x68"),
    ("head_fused", _with(_head_fused, "pair_swapped"), "head_fused", "pair copy"),
)
DEFECT_IDS = [d[0] + (" " + d[1].defect if isinstance(getattr(d[1], "defect", None), str) else "") for d in DEFECTS]


@pytest.mark.parametrize("name,variant,family,must_fail", DEFECTS, ids=DEFECT_IDS)
def test_planted_defect_fails_its_row_and_only_its_operator(clean, name, variant, family, must_fail):
    touched = [(title, check) for title, check in op_checks.CHECKS if name in clean[title][1]]
    assert touched  # (a check that never calls the operator cannot change: its rows are the clean ones, which pass)
    failed = []
    for title, check in touched:
        with torch.no_grad():
            failed += [r for r in check(CPU, Recorder(**{name: variant})) if not _passes(r)]
    assert any(r.op == family and must_fail in r[0] for r in failed), [r[0] for r in failed]
    assert all(r.op == family for r in failed), [r[0] for r in failed if r.op != family]


# ----------------------------------------------------------------------------------------- 4. the convolution forms
def test_conv_forms_matrix_is_complete(clean):
    """Every id has an accepted row for every form that applies to its stride (the rule the GPU tests assert), the only refusals
    are the LDS-DMA members' on W % 4 != 0, every transposed-convolution id has both of its guarded rows, and each planted defect
    above fails rows of its own form only."""
    lib = op_checks.conv_lib()
    rows = clean["op conv epilogue forms"][0]
    ids = list(range(lib.drba_conv3x3_num_cfgs()))
    assert len(ids) == 38 and not op_checks.conv_forms_missing(rows, lib, ids)
    assert len(op_checks.CONV_FORMS) == 12 and len({f.name for f in op_checks.CONV_FORMS}) == 12
    assert not [r[0] for r in rows if getattr(r, "kind", None) == "error"]
    for ps in (0, 1):
        assert {r.cfg for r in rows if getattr(r, "form", None) == "deconv" and r.kind == "guard" and f"ps={ps}" in r[0]} == set(range(15))
    assert {r.cfg for r in rows if getattr(r, "kind", None) == "nonfinite"} == set(ids)
    guarded = {(r.cfg, r.form) for r in rows if getattr(r, "kind", None) == "guard" and r.form not in ("deconv", "shuffle")}
    assert guarded == {(r.cfg, r.form) for r in rows if getattr(r, "kind", None) == "value" and r.form not in ("deconv", "shuffle")}


def test_conv_form_defects_fail_rows_of_their_form_only():
    lib = op_checks.conv_lib()
    ids = [min(c for c in range(lib.drba_conv3x3_num_cfgs()) if op_checks.conv_id_class(lib, c) == cls) for cls in op_checks.CONV_PAIRS]
    for defect, form in (("res2_dropped", "pre+res+res2"), ("beta_order", "resconv"), ("post_slope_02", "bias+prelu(0.1)"), ("pre_on_residual", "pre+res=in")):
        with torch.no_grad():
            rows = op_checks.check_conv_forms(CPU, Recorder(Conv3x3=_conv_defect(defect)), cfgs=ids)
        failed = [r for r in rows if not _passes(r)]
        assert failed and all(r.form.startswith(form) for r in failed), (defect, [r[0] for r in failed])
        hit = {r.cfg for r in failed}
        s2 = {c for c in ids if op_checks.conv_id_class(lib, c) == "s2"}  # (the forms with a residual have no stride-2 rows)
        assert hit == set(ids) - (s2 if form not in op_checks.CONV_PLAIN_FORMS else set()), (defect, hit)


def test_conv_many_rows_on_a_small_batch():
    """check_conv_many's rows with the stand-in at N = 4: clean, and failing in the form whose operand a defect touches"""
    with torch.no_grad():
        rows = op_checks.check_conv_many(CPU, Recorder(), n=4)
        assert len(rows) == 2 * len(op_checks.conv_many_ids(op_checks.conv_lib())) and all(_passes(r) for r in rows), [r[0] for r in rows if not _passes(r)]
        for defect, form in (("res2_dropped", "pre+res+res2"), ("beta_order", "resconv res is in")):
            bad = [r for r in op_checks.check_conv_many(CPU, Recorder(Conv3x3=_conv_defect(defect)), n=4) if not _passes(r)]
            assert bad and all(r.form == form for r in bad) and len(bad) == len(rows) // 2, (defect, [r[0] for r in bad])


# ----------------------------------------------------------------------------------------- 5. the transformer rows reach what they name
def test_transformer_row_lists_reach_every_dispatch_form():
    """From the restated host rules (op_checks.attn16_ksplit, attn_ksplit, gcorr_ksplit, LIN_WIDE_MIN): the row lists hold every
    key-run count the rules can choose, uneven splits, both wave forms, both sides of every tile, and the two linear tile forms.  The
    GPU tests read the same from the kernel trace."""
    oc = op_checks
    runs2 = {k: min(c.L for c in oc.ATTN_RUNS if oc.attn_runs(c, 2) == k) for k in {oc.attn_runs(c, 2) for c in oc.ATTN_RUNS}}
    assert set(runs2) == {1, 2, 3, 4, 5, 6} and {oc.attn_runs(c, 3) for c in oc.ATTN_RUNS} == {1, 2, 4}
    first = {}
    for L in range(1, 4200):
        first.setdefault(oc.attn16_ksplit(1, L, oc.attn16_waves(L)), L)
    assert first == {1: 1, 2: 449, 3: 705, 4: 961, 5: 2113, 6: 4161}  # the rule's own thresholds for one window
    assert all(first[k] <= runs2[k] < first[k] + 64 for k in (2, 3, 4, 5, 6))  # each count at the smallest chunk count that gives it
    assert sum(oc.uneven(c.L, oc.attn_runs(c, 2)) for c in oc.ATTN_RUNS) >= 2 and sum(oc.uneven(c.L, oc.attn_runs(c, 3)) for c in oc.ATTN_RUNS) >= 2
    assert {oc.attn16_waves(c.L) for c in oc.ATTN_CASES} == {4, 8} and {187, 192, 195} <= {c.L for c in oc.ATTN_GEOMETRY}
    assert {63, 64, 65, 127, 128, 129, 255, 256, 257, 70} <= {c.L for c in oc.ATTN_GEOMETRY}
    assert {1, 4, 9, 16, 18} <= {c.nwin for c in oc.ATTN_GEOMETRY}
    assert any(c.w // c.splits == 1 and c.L > 64 and not c.shift for c in oc.ATTN_GEOMETRY)
    assert any(c.shift and (c.h // c.splits) % 2 and (c.w // c.splits) % 2 for c in oc.ATTN_GEOMETRY)
    assert any(c.b == 2 and c.shift and oc.attn_runs(c, 2) > 1 and oc.attn_runs(c, 3) > 1 for c in oc.ATTN_GEOMETRY)
    assert [c.L for c in oc.ATTN_TABLE] == [oc.ATTN_TAB_CAP, oc.ATTN_TAB_CAP + 64, oc.ATTN_TAB_CAP + 64] and oc.ATTN_TABLE[2].shift  # the last walk that takes the table, the first that cannot
    got = {oc.gcorr_ksplit(h * w) for h, w in oc.GCORR_RUNS} | {oc.gcorr_ksplit(h * w) for h, w in oc.GCORR_MAPS}
    assert got == {1, 2, 3, 4, 5, 6, 7, 8}
    first = {}
    for L in range(1, 2100):
        first.setdefault(oc.gcorr_ksplit(L), L)
    assert first == {1: 1, 2: 449, 3: 705, 4: 961, 5: 1217, 6: 1473, 7: 1729, 8: 1985}
    # every count at the smallest chunk count that gives it -- even runs of the minimum of 4 chunks -- on a ragged map (L no multiple of 64)
    smallest = {k: min(h * w for h, w in oc.GCORR_RUNS if oc.gcorr_ksplit(h * w) == k) for k in range(2, 9)}
    assert all(first[k] <= smallest[k] < first[k] + 64 and smallest[k] % 64 and -(-smallest[k] // 64) == 4 * k for k in range(2, 9)), smallest
    assert len(set(oc.GCORR_MAPS + oc.GCORR_RUNS)) == len(oc.GCORR_SEEDS) == len(oc.GCORR_MAPS) + len(oc.GCORR_RUNS)
    assert sum(oc.uneven(h * w, oc.gcorr_ksplit(h * w)) for h, w in oc.GCORR_RUNS) >= 3
    assert {h * w for h, w in oc.GCORR_MAPS} >= {63, 64, 65, 127, 128, 129, 70} and (1, 70) in oc.GCORR_MAPS and (70, 1) in oc.GCORR_MAPS
    k, n = oc.LIN_WIDE_KN
    wgs = [-(-m // 128) * -(-n // 128) for m, _ in oc.LIN_WIDE]
    assert wgs == [1536, 1504] and [w >= oc.LIN_WIDE_MIN for w in wgs] == [wide for _, wide in oc.LIN_WIDE] and oc.LIN_WIDE[0][0] % 128
    ms, ns, ks = ({c[i] for c in oc.LIN_EDGES} for i in (0, 2, 1))
    assert ms == {1, 15, 16, 17, 63, 64, 65, 127, 128, 129} and ns == {1, 15, 16, 17, 40, 127, 128, 129, 384} and ks == {32, 64, 128}
    assert {c[3] for c in oc.LIN_EDGES} == {True, False} and any(c[2] == 129 and c[3] for c in oc.LIN_EDGES)


def test_restated_attention_rules_match_the_library():
    """drba_window_attention_ws_floats / drba_global_expect2_ws_floats are host functions of the library (no device): the restated
    rules give the same workspace sizes, i.e. the same larger run count, for every row of the lists and along a sweep of L"""
    lib, oc = op_checks.conv_lib(), op_checks
    shapes = [(c.b, c.h, c.w, c.splits) for c in oc.ATTN_CASES + oc.ATTN_TABLE] + [(b, 1, L, 1) for L in range(1, 4300, 7) for b in (1, 8)]
    for b, h, w, s in shapes:
        nwin, L = b * s * s, (h // s) * (w // s)
        ks = max(oc.attn_ksplit(nwin, L), oc.attn16_ksplit(nwin, L, oc.attn16_waves(L)))
        assert lib.drba_window_attention_ws_floats(b, h, w, s) == (nwin * L * ks * 132 if ks > 1 else 0), (b, h, w, s)
    for L in list(range(1, 2200, 3)) + [h * w for h, w in oc.GCORR_RUNS + oc.GCORR_MAPS] + [8640]:
        ks = oc.gcorr_ksplit(L)
        assert lib.drba_global_expect2_ws_floats(L) == (L * ks * 4 if ks > 1 else 0), L


def test_peaked_rows_are_decisive(clean):
    """the mask rows move by >= 100 tolerances in >= 2 % of their rows under a -inf mask; the late-maximum rows have their maximum in
    the last chunk (asserted in op_checks.attn_refs / gcorr_refs before anything runs; the figures are in the rows)"""
    rows = clean["op window attention edges"][0]
    masks = [c for c in op_checks.ATTN_PEAKED if c.kind == "mask"]
    assert len(masks) >= 2 and any((c.h // c.splits) % 2 for c in masks)
    for c in masks:
        r = op_checks.attn_refs(c)
        assert r["mask_share"] >= 0.02 and r["mask_diff"] >= 100 * max(row[2] for row in rows if getattr(row, "case", None) == c)
    late = [c for c in op_checks.ATTN_PEAKED if c.kind == "late"]
    assert late and all(i // 64 == -(-c.L // 64) - 1 for c in late for i in op_checks.attn_refs(c)["late_argmax"])
    # on the inputs of the older check (amplitude 1.5, scale sqrt(128)) the mask value is invisible: what these rows are for
    plain = next(c for c in op_checks.ATTN_GEOMETRY if (c.h, c.w, c.splits, c.shift) == (22, 34, 2, True))
    q, k, v = (t.double() for t in op_checks.attn_inputs(plain))
    assert float((op_checks.attn_ref(q, k, v, plain, float("-inf")) - op_checks.attn_refs(plain)["ref64"]).abs().max()) < 1e-12


# ----------------------------------------------------------------------------------------- 6. the fused encoder's rows
def _head_failed(defect):
    with torch.no_grad():
        rows = op_checks.check_head_fused(CPU, Recorder(head_fused=_with(_head_fused, defect)))
    return rows, [r for r in rows if not _passes(r)]


def test_head_case_table_reaches_every_edge(clean):
    """The case table's edge conditions, recomputed from H, W and the tile constants (op_checks asserts the table against them at
    import), every shape and input kind among the rows in both forms, and the two-term rows' format floor below the one rule."""
    oc = op_checks
    assert [c[:2] for c in oc.HEAD_CASES] == [(2, 4), (6, 12), (16, 64), (18, 68), (22, 76), (38, 140), (40, 144), (16, 516), (130, 4)]
    by = {c[:2]: oc.head_edges(*c[:2]) for c in oc.HEAD_CASES}
    assert "interior" in by[(38, 140)] and "W%8==4" in by[(38, 140)] and "interior" in by[(40, 144)] and "W%8==4" not in by[(40, 144)]
    assert not any("interior" in oc.head_edges(h - 2, w) or "interior" in oc.head_edges(h, w - 4) for h, w in ((38, 140),))  # the smallest such frame
    assert "tiles_x>8" in by[(16, 516)] and "tiles_y>8" in by[(130, 4)] and "ring" in by[(22, 76)] and "W%8==4" in by[(18, 68)]
    assert all(by[s] == {"one tile", "W%8==4"} for s in ((2, 4), (6, 12))) and by[(16, 64)] == {"one tile"}
    rows = clean["op fused encoder"][0]
    names = [r[0] for r in rows]
    for form in ("fp32", "two-term"):
        for h, w, _ in oc.HEAD_CASES:
            assert sum(f"{form} rand {h}x{w}:" in n for n in names) == 5, (form, h, w)
        for h, w in oc.HEAD_EXTRA:
            for kind in ("zero frame", "randn*1e3", "randn*1e-3"):
                assert sum(f"{form} {kind} {h}x{w}:" in n for n in names) == 5, (form, kind, h, w)
        assert sum(n.startswith(f"head_fused {form} [") and "is not taken" in n for n in names) == len(oc.HEAD_REFUSED)
    assert sum("fp32 NaN pixel 38x140:" in n for n in names) == 5 and not any("two-term NaN" in n for n in names)
    assert any("carries the pair tag" in n and " 2x4:" in n for n in names)
    two = [r for r in rows if getattr(r, "two", False)]
    assert len(two) == len(oc.HEAD_CASES) + 3 * len(oc.HEAD_EXTRA)
    for r in two:  # no second bar for the two-term form: what the format can hold stays well inside the rule
        assert 3.0 * r.fmt_floor <= r[2] and r[2] == oc.rule_tol(r.refmax, r.floor), (r[0], r.fmt_floor, r[2])
    big = [r for r in rows if "randn*1e3" in r[0] and r.refmax is not None]
    assert big and all(1e3 < r.refmax < 65504 for r in big)  # far below the two-term form's documented 65504 * 16


def test_head_nan_pixel_reaches_the_cone_of_four_tiles():
    """One NaN at channel 1, pixel (15, 63) of 38 x 140: the reference is NaN in exactly rows 9..22 x columns 57..70 of all 16
    channels, in float64 and in float32, across the seam of tiles (0, 0), (0, 1), (1, 0), (1, 1), and finite everywhere else."""
    oc = op_checks
    h, w = oc.HEAD_NAN[:2]
    r = oc.head_refs(h, w, "NaN pixel")
    assert int(r["x"].isnan().sum()) == 1 and bool(r["x"][0, oc.HEAD_NAN[2], oc.HEAD_NAN[3], oc.HEAD_NAN[4]].isnan())
    (ra, rb), (ca, cb) = oc.HEAD_NAN_CONE
    want = torch.zeros(1, 16, h, w, dtype=torch.bool)
    want[:, :, ra:rb + 1, ca:cb + 1] = True
    for ref in (r["ref64"], r["ref32"]):
        assert torch.equal(ref.isnan(), want) and bool(torch.isfinite(ref[~want]).all())
    assert ra < 16 <= rb and ca < 64 <= cb  # both sides of the 16 x 64 tile seam, on both axes


def test_head_window_defect_needs_more_than_one_tile():
    """A frame window one pixel short is invisible where there is one tile (2x4, 6x12, 16x64) and on a zero frame; every rand row of a
    frame with more than one tile fails its value row -- what the multi-tile shapes are in the list for."""
    rows, failed = _head_failed("window_one_short")
    bad = {r[0] for r in failed}
    assert all(r.op == "head_fused" and "planar vs fp64" in r[0] for r in failed), sorted(bad)
    for form in ("fp32", "two-term"):
        for h, w, edges in op_checks.HEAD_CASES:
            hit = f"head_fused {form} rand {h}x{w}: planar vs fp64" in bad
            assert hit == ("one tile" not in edges), (form, h, w, hit)
        assert not any(f"{form} zero frame" in n for n in bad)
    assert all(r[1] > 1000 * r[2] for r in failed if " rand " in r[0])  # (a 1e-3 frame moves by ~10 tolerances: the bias dominates it)


def test_head_tail_defect_fails_exactly_the_w4_shapes():
    rows, failed = _head_failed("tail_unwritten")
    shapes = {(h, w) for h, w, e in op_checks.HEAD_CASES if "W%8==4" in e}
    hit = {(h, w) for h, w, _ in op_checks.HEAD_CASES if any(f" {h}x{w}:" in r[0] for r in failed)}
    assert hit == shapes and (40, 144) not in hit and (16, 64) not in hit, sorted(hit)
    assert not any("planar=False == the pair copy" in r[0] for r in failed)  # the pair layout is stored from the same registers, whole


def test_head_pair_defect_fails_no_value_row():
    rows, failed = _head_failed("pair_swapped")
    assert failed and all(r[2] == 0.0 and r.floor is None for r in failed), [r[0] for r in failed if r[2] != 0.0]
    n_inputs = sum(len(forms) for *_, forms in op_checks.head_inputs())
    assert sum("pair copy == the pair layout" in r[0] for r in failed) == n_inputs == sum("features_planar" in r[0] for r in failed)


def test_token_table_rows_with_the_standin():
    """the three C-ABI rows of the GPU suite (3968 and 4032 keys in one walk, and four shifted windows of 4032) on the CPU: the
    stand-in holds their fp64 rows"""
    for c in op_checks.ATTN_TABLE:
        q, k, v = op_checks.attn_inputs(c)
        with torch.no_grad():
            row = op_checks.attn_row("window_attention", c, 2, _window_attention(q, k, v, c.h, c.w, c.splits, c.shift, c.scale))
        assert _passes(row), row


# ----------------------------------------------------------------------------------------- 8. the fused RIFE splats
RIFE_TITLE = "op fused RIFE splats"
ALONE_MIN = 1e3         # a source of an "alone" background: its flow leaves the map (it is long, and lands nowhere)
RIFE_NOMAP_WORDS = 64  # the reach map of the stand-in that runs the no-map rows here: N = 4 items of 16 / 17 tiles
RIFE_DEFECTS = (  # (the stand-in's changed rule, the case group that must fail, part of the name of a row that must fail)
    ("window_one_short", "window", "window R="),          # sources at the far window column / row dropped
    ("reach_too_tight", "reach", "reach rounding"),        # the reach of a positive flow as floor(f): one pixel short (see reach_tight below)
    ("own_reach_only", "neighbour", "neighbour reach"),    # the 3 x 3 neighbourhood ignored
    ("spill_dropped", "capacity", "capacity CAP+1"),       # records at or beyond kCAP lost
    ("spill_all_corners", "capacity", "capacity CAP+1"),   # a spilled straddling record adds the corners the neighbour owns, too
    ("stale_dirty", "long", "non-zero workspace words"),   # a flag left set
    ("item0_reach", "items", "item 3 of 8"),               # every item reads item 0's reach entries
)


def _rife_ns(defect=None, reach_words=det_common.REACH_WORDS):
    return Recorder(**_RifeSplats(defect, reach_words).namespace())


def _rife_cases_with_inputs():
    """(case name, group, op, t, flow_self, flow_other, planted, claims) of every row's inputs: the table, the capacity rows, the items"""
    out = []
    for case in op_checks.rife_cases():
        for op, t in op_checks.RIFE_FLOW + (op_checks.RIFE_DRM if case.drm_flow is not None else ()):
            out.append((case.name, case.group, op, t) + op_checks.rife_case_inputs(case, op, t) + (case.planted, case.claims))
    for label, total, _, drm in op_checks.CAPACITY_TOTALS:
        for op, t in op_checks.RIFE_FLOW + (op_checks.RIFE_DRM if drm else ()):
            fs, fo, planted = op_checks.capacity_inputs(label, op, t)
            out.append((f"capacity {label}", "capacity", op, t, fs, fo, planted, {"records": total}))
    f, planted = op_checks.rife_item_flow()
    out.append(("items", "items", "flow_reverse", None, f, None, planted, {}))
    return out


@pytest.mark.parametrize("defect,group,must_fail", RIFE_DEFECTS, ids=[d[0] for d in RIFE_DEFECTS])
def test_rife_planted_defect_fails_its_case_and_only_this_operator(clean, defect, group, must_fail):
    with torch.no_grad():
        failed = [r for r in op_checks.check_rife_splats(CPU, _rife_ns(defect)) if not _passes(r)]
    assert any(r.group == group and must_fail in r[0] for r in failed), [r[0] for r in failed]
    assert all(r.op == op_checks.RIFE_OP for r in failed)
    fused = set(_RifeSplats().namespace())  # no other family calls a fused entry point: its rows are the clean ones
    assert all(not (fused & used) for title, (_, used) in clean.items() if title != RIFE_TITLE)
    if defect == "window_one_short":  # per halo variant, on both backgrounds, in both modes
        for R in (4, 8, 16):
            for bg in ("alone", "identity"):
                for tag in ("", " det"):
                    assert any(f"window R={R} {bg} 100x200{tag}:" in r[0] for r in failed), (R, bg, tag)
    if defect in ("spill_dropped", "spill_all_corners"):  # at kCAP and below nothing spills: those rows hold
        assert not any("capacity CAP:" in r[0] or "capacity CAP det:" in r[0] or "capacity CAP-1" in r[0] for r in failed), [r[0] for r in failed]
        assert any("capacity 1.5 CAP" in r[0] for r in failed)


def test_rife_reach_from_floor_plus_one_is_a_correct_tightening():
    """The pre-pass rounds the reach of a positive flow to floor(f) + 2.  floor(f) + 1 ("reach_tight") still covers the footprint: its
    far corner is x + floor(f) + 1, and the window of halo R begins at tx0 - R.  The rows must tell that tightening (every row
    passes) from floor(f), which loses the far column ("reach_too_tight", above) -- they do not assert the path, only the values."""
    with torch.no_grad():
        rows = op_checks.check_rife_splats(CPU, _rife_ns("reach_tight"))
    assert all(_passes(r) for r in rows), [r[0] for r in rows if not _passes(r)]
    flow = op_checks.rife_cases(("reach",))[0].flow
    assert not torch.equal(det_common.tile_variant(flow), det_common.tile_variant(flow, tight=1))  # (the tightening does change variants here)


def test_rife_nomap_rows_on_a_small_reach_map():
    """check_rife_splats_nomap's rows with stand-ins whose reach map has 64 words: clean; the launch that skips the map scanning
    the 4-pixel halo fails the rows of that launch only.  And the geometry the GPU suite runs, from the restated constants."""
    rw = RIFE_NOMAP_WORDS
    with torch.no_grad():
        rows = op_checks.check_rife_splats_nomap(CPU, _rife_ns(None, rw), reach_words=rw)
        bad = [r for r in op_checks.check_rife_splats_nomap(CPU, _rife_ns("no_map_as_r4", rw), reach_words=rw) if not _passes(r)]
    assert len(rows) >= 2 * 2 * 2 * (3 * 4 + 2) and all(_passes(r) for r in rows), [r[0] for r in rows if not _passes(r)]
    assert bad and all("(without the reach map)" in r[0] and r.op == op_checks.RIFE_OP for r in bad), [r[0] for r in bad]
    assert any(" det" in r[0] and "== two chunks" in r[0] for r in bad) and any("item 0" in r[0] for r in bad)
    for words in (rw, det_common.REACH_WORDS):
        (n, h), (n2, h2) = op_checks.nomap_geometry(words, True), op_checks.nomap_geometry(words, False)
        tiles, tiles2 = det_common.tiles_of(h, op_checks.NOMAP_W), det_common.tiles_of(h2, op_checks.NOMAP_W)
        assert tiles[1] == tiles2[1] == 1 and n == n2 and n * tiles[0] == words and n2 * tiles2[0] == words + n
        assert (n // 2) * tiles2[0] <= words  # the chunks use the map
    assert n * h * op_checks.NOMAP_W < 12.7e6 and h2 < 65536
    for with_map in (True, False):  # the two launches take different halo variants, and the planted sources are what they claim
        n, h = op_checks.nomap_geometry(rw, with_map)
        f, planted = op_checks.nomap_flow(n, h, 3900 + int(with_map))
        v = det_common.tile_variant(f, use_map=with_map)
        assert set(v.unique().tolist()) == ({4, 16} if with_map else {16})
        assert float((det_common.tile_variant(f, use_map=True) == 4).float().mean()) > 0.5
        finite, short = det_common.source_class(f)
        assert int((finite & ~short).sum()) >= 9 and int((~finite).sum()) >= 6 and int((det_common.source_reach(f) == 16).sum()) >= 6
        _assert_decisive("nomap", "flow_reverse", None, f, None, planted)


def _loo_effect(op, t, fs, fo, planted):
    """per planted source: the largest change of the reference's output over the pixels of its footprint when that source alone is
    taken out -- from the fp64 sums of the reference (value * weight and weight per pixel), minus the source's own terms"""
    n, _, h, w = fs.shape
    flow = op_checks.rife_splat_flow(op, fs, fo, t)
    val = fs if op == "flow_reverse" else op_checks.rife_u(op, fs, fo, t)
    nv = val.shape[1]
    sums = op_checks.softsplat_ref(torch.cat([val, torch.ones_like(val[:, :1])], 1), flow, None, "sum")
    tgt = op_checks._grid32(h, w) + flow

    def value(num, den, k, py, px):
        if den / (den + 1e-7) < 0.999:
            return [2.0 * max(h, w)] * nv if op == "flow_reverse" else [float(val[k, 0, py, px])]
        return [(-2.0 if op == "flow_reverse" else 1.0) * float(a) / (den + 1e-7) for a in num]

    out = []
    for k, y, x in planted:
        X, Y = float(tgt[k, 0, y, x]), float(tgt[k, 1, y, x])
        assert abs(X) < 2.0 ** 30 and abs(Y) < 2.0 ** 30, (k, y, x)  # (a planted source is one that contributes)
        x0, y0 = int(X // 1), int(Y // 1)
        eff = 0.0
        for dy in (0, 1):
            for dx in (0, 1):
                px, py = x0 + dx, y0 + dy
                if not (0 <= px < w and 0 <= py < h):
                    continue
                wgt = ((X - x0) if dx else (x0 + 1 - X)) * ((Y - y0) if dy else (y0 + 1 - Y))
                num, den = sums[k, :nv, py, px], float(sums[k, nv, py, px])
                before = value(num, den, k, py, px)
                after = value(num - val[k, :, y, x].double() * wgt, den - wgt, k, py, px)
                eff = max([eff] + [abs(a - b) for a, b in zip(before, after)])
        out.append(eff)
    return out


def _assert_decisive(name, op, t, fs, fo, planted):
    eff = _loo_effect(op, t, fs, fo, planted)
    weak = [(p, e) for p, e in zip(planted, eff) if not e >= 100.0 * op_checks.RIFE_BARS[op]]
    assert not weak, (name, op, t, weak[:5])
    return len(eff)


def test_rife_planted_sources_are_decisive():
    """Leave-one-out: the reference without a planted source differs from the reference by at least 100 tolerances at some pixel,
    for every planted source of every row -- none is one whose loss the row would forgive."""
    n = sum(_assert_decisive(name, op, t, fs, fo, planted) for name, _, op, t, fs, fo, planted, _ in _rife_cases_with_inputs())
    assert n > 500, n


def test_rife_rows_are_stable_enough(clean):
    """the unstable share of every row, from the reference alone, is under decisions.UNSTABLE_SHARE -- and a map of one pixel has none"""
    from tests import decisions
    shares = [r for r in clean[RIFE_TITLE][0] if "unstable share" in r[0]]
    assert len(shares) > 100 and all(r[1] <= decisions.UNSTABLE_SHARE == r[2] for r in shares), [r[0] for r in shares if r[1] > r[2]]
    assert all(r[1] == 0.0 for r in shares if "small 1x1" in r[0])
    bars = {r[2] for r in clean[RIFE_TITLE][0] if ": stable pixels" in r[0] or "nearer branch" in r[0]}
    assert bars == {2e-4, 2e-5}  # the two bars gpu_checks.check_glue holds these entry points to


REACH_EXPECTED = (4, 5, 4, 5, 4, 8, 9, 8, 9, 8, 16, None, 16, 16, None, 2, 6, 10, 5, 9)  # per REACH_VALUES; None: long


def test_rife_case_table_reaches_what_it_names():
    """From the restated rules (tests/det_common.py), on the flow every entry point splats along: the window rows take exactly
    their variant at both tiles; the reach rows hold every rounding on both sides of 4, 8 and 16 and both long bounds; a quiet tile
    has reach 0 and scans 16; long, non-finite and far sources are where the rows say; the record totals are exactly those claimed
    and the spilled records straddle the tile edge; every item has its pinch, its long block, its reach-16 tile and the quiet one."""
    TX, TY, CAP = det_common.TX, det_common.TY, det_common.CAP
    seen = set()
    for name, group, op, t, fs, fo, planted, claims in _rife_cases_with_inputs():
        flow = op_checks.rife_splat_flow(op, fs, fo, t)
        finite, short = det_common.source_class(flow)
        variant, reach = det_common.tile_variant(flow), det_common.tile_reach(flow)
        seen.add(group)
        if group == "window":
            for tx, ty in claims["tiles"]:
                assert int(variant[0, ty, tx]) == claims["variant"], (name, op, t, tx, ty)
            assert all(bool(finite[p] & short[p]) for p in planted) and len(planted) >= 30
            if "identity" in name:
                assert set(reach.unique().tolist()) <= {2, claims["variant"]}
        elif group == "reach":
            assert len(REACH_EXPECTED) == len(claims["values"])
            r = det_common.source_reach(flow)
            for i, (k, y, x) in enumerate(planted):
                want = REACH_EXPECTED[i // 4]
                assert bool(finite[k, y, x]) and bool(short[k, y, x]) == (want is not None) and int(r[k, y, x]) == (want or 0), (i, k, y, x)
                assert int(reach[k].max()) == (want or 0)  # the item's only source
        elif group == "neighbour":
            for k, (tx, ty) in claims["quiet"].items():
                assert int(reach[k, ty, tx]) == 0 and int(variant[k, ty, tx]) == 16 and int(reach[k].max()) == 16, (k, tx, ty)
            k = claims["mirror"]
            tot = det_common.tile_record_totals(flow)[k]
            assert int(reach[k, 1, 1]) == 16 and bool((variant[k] == 16).all()) and int(tot.sum()) == int(tot[1, 1]) == 2
        elif group == "long":
            assert int((finite & ~short).sum()) == claims["long"] + (0 if claims["long"] == 0 else int((flow[:, 0] >= ALONE_MIN).sum()))
            if claims["long"]:
                tg = op_checks._grid32(*flow.shape[2:]) + flow[0]
                for _, y, x in planted:  # exactly one corner of the footprint inside the map
                    cx, cy = int(tg[0, y, x].floor()), int(tg[1, y, x].floor())
                    inside = [(a, b) for a in (cx, cx + 1) for b in (cy, cy + 1) if 0 <= a < flow.shape[3] and 0 <= b < flow.shape[2]]
                    assert len(inside) == 1 and not bool(short[0, y, x]), (y, x, inside)
        elif group == "nonfinite":
            ys, xs = zip(*claims["spots"])
            assert int((~finite[0, list(ys), list(xs)]).sum()) == 6 and int((finite & ~short)[0, list(ys), list(xs)].sum()) == 12
        elif group == "capacity":
            tot = det_common.tile_record_totals(flow)
            tx, ty = op_checks.PINCH
            assert int(tot[0, ty, tx]) == claims["records"], (name, op, t)
            kx, ky, ok = det_common.record_keys(flow)
            mine = ok[0] & (kx[0] >= tx * TX - 1) & (kx[0] <= tx * TX + 31) & (ky[0] >= ty * TY - 1) & (ky[0] <= ty * TY + 15)
            assert int(mine.sum()) == claims["records"]
            last = ky[0][mine].max()  # the records in the last key row spill first
            assert int(last) == ty * TY + 15 and int((mine & (ky[0] == last)).sum()) >= 2 and int((mine & (ky[0] == ty * TY - 1)).sum()) >= 2
            assert ("long source" in name) == bool((finite & ~short & (flow[:, 0].abs() < 1e3)).any())
        elif group == "items":
            tot = det_common.tile_record_totals(flow)
            for k in range(op_checks.ITEMS):
                (ax, ay), (qx, qy), (px, py) = op_checks.ITEM_REACH16[k], op_checks.ITEM_REACH16[k - 1], op_checks.ITEM_PINCH[k]
                assert int(reach[k, ay, ax]) == 16 and int(reach[k, qy, qx]) == 0 and int(reach[k - 1, qy, qx]) == 16, k
                assert int(tot[k, py, px]) > CAP and int((finite & ~short)[k].sum()) == 36, (k, int(tot[k, py, px]))
                assert len({op_checks.ITEM_PINCH[k], op_checks.ITEM_REACH16[k], op_checks.ITEM_REACH16[k - 1]}) == 3
            assert len(set(op_checks.ITEM_PINCH)) == len(set(op_checks.ITEM_REACH16)) == op_checks.ITEMS
    assert seen == set(op_checks.RIFE_GROUPS)
    assert [tuple(c.flow.shape[2:]) for c in op_checks.rife_cases(("small",))] == list(op_checks.RIFE_SIZES)
    totals = {c[1] for c in op_checks.CAPACITY_TOTALS}
    assert {CAP - 1, CAP, CAP + 1} <= totals and any(abs(v - 1.5 * CAP) < 1 for v in totals)

