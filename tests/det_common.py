"""Inputs and CPU-side conditions shared by tests/test_gpu_deterministic.py: flows at 70 x 100 (5 x 4 output tiles of 32 x 16, ragged on
both edges) that together reach every path of the fused splats, and the share of output pixels whose sum has more than one term.
Below them, the host-visible rules of the fused splats' kernels restated (source class, reach, halo variant, records per tile): what
tests/op_checks.py chooses and asserts the cases of the fused RIFE splats with."""
import functools

import numpy as np
import torch

H, W = 70, 100
TX, TY, CAP, RMAX = 32, 16, 1536, 16  # splat_warp.hip: kSX, kSY, kCAP, kRMax
REACH_WORDS = 1 << 18                  # kReachWords: the reach map in front of the fused splats' workspace (scratch)
PINCH_TILE = (1, 1)                    # the tile (x 32..63, y 16..31) the contracted patch is pulled into


def _noise(g, bound, h=H, w=W):
    """Normal noise times per-pixel magnitudes spread over three decades (so that the order of a sum shows in its last bits),
    kept strictly inside |f| < bound."""
    mag = 10.0 ** (torch.rand(1, 1, h, w, generator=g) * 3.0 - 3.0) * bound  # bound * [1e-3, 1)
    return (torch.randn(1, 2, h, w, generator=g) * mag).clamp(-bound * 0.999, bound * 0.999)


@functools.lru_cache(maxsize=None)
def flows():
    """name -> [1, 2, H, W] flow, and the other direction's flow of the DRM entry points."""
    g = torch.Generator().manual_seed(2024)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = {"noise3": _noise(g, 3.0), "noise7": _noise(g, 7.0), "noise15": _noise(g, 15.0)}  # the three halo variants (4, 8, 16)
    longf = _noise(g, 3.0)
    longf[:, :, 20:50, 10:40] += 40.0 * torch.sign(torch.randn(1, 2, 30, 30, generator=g))  # 40-pixel flows: the long pre-pass
    out["long"] = longf
    # a 48 x 48 patch contracted towards the centre of one tile.  By 0.6, not the 0.8 first planned: at 0.8 the patch's outer ring has
    # |flow| up to 19 -- beyond the 16-pixel halo, i.e. long sources that never become records of the tile (1518 records counted for
    # that tile, under kCAP = 1536) -- while at 0.6 all 2304 sources are short and land within 10 pixels of the centre
    cx, cy = PINCH_TILE[0] * TX + TX / 2 - 0.5, PINCH_TILE[1] * TY + TY / 2 - 0.5
    pinch = _noise(g, 3.0) * 0.1
    py, px = slice(int(cy - 23.5), int(cy - 23.5) + 48), slice(int(cx - 23.5), int(cx - 23.5) + 48)
    pinch[0, 0, py, px] += -0.6 * (xs[py, px] - cx)
    pinch[0, 1, py, px] += -0.6 * (ys[py, px] - cy)
    out["pinch"] = pinch
    nanf = _noise(g, 7.0)
    nanf[0, 0, 7, 9], nanf[0, 1, 30, 60], nanf[0, 0, 69, 99], nanf[0, 1, 0, 0] = float("nan"), float("inf"), float("-inf"), float("nan")
    out["nan"] = nanf
    other = _noise(g, 7.0)
    return {k: v.contiguous() for k, v in out.items()}, other.contiguous()


def other_for(name):
    """The other direction's flow of a DRM case.  The pinch keeps its contraction and the long region its 40 pixels only if u stays
    near 1: a far larger other flow makes the ratio d_other / (d_self + d_other) ~ 0.999."""
    fl, other = flows()
    return fl[name] * 1000.0 + 1.0 if name in ("pinch", "long") else other


def splat_flow(op, f_self, f_other, t, eps=1e-4):
    """The flow an entry point splats along, on the CPU in fp32: the flow itself (flow_reverse) or self * u with the linear
    u = r * t * 2 / the retimed u = get_drm_t(r, t), r = d_other / (d_self + d_other)."""
    if op == "flow_reverse":
        return f_self
    from tests import decisions
    _, r = decisions._ratio_maps(f_self, f_other, eps)
    return f_self * (r * t * 2 if op == "drm_rife_linear" else decisions._retime(r, t, False))


def key_counts(flow):
    """Records per key of the (H + 1) x (W + 1) grid of footprint origins, from the flow alone (one image)."""
    f = flow[0].double().numpy()
    h, w = f.shape[1:]
    ys, xs = np.mgrid[0:h, 0:w]
    X, Y = xs + f[0], ys + f[1]
    ok = np.isfinite(X) & np.isfinite(Y)
    fx, fy = np.floor(np.where(ok, X, -9)), np.floor(np.where(ok, Y, -9))
    ok &= (fx >= -1) & (fx <= w - 1) & (fy >= -1) & (fy <= h - 1)
    cnt = np.zeros((h + 1, w + 1), dtype=np.int64)
    np.add.at(cnt, (fy[ok].astype(int) + 1, fx[ok].astype(int) + 1), 1)
    return cnt, (fx, fy, ok)


def multi_term_share(flow):
    """Share of output pixels that read at least one key segment holding two or more records: only those sums have an order."""
    cnt, _ = key_counts(flow)
    m = cnt >= 2
    return float((m[:-1, :-1] | m[:-1, 1:] | m[1:, :-1] | m[1:, 1:]).mean())


def tile_records(flow, tile):
    """Records the tile kernel holds for output tile `tile` = (tx, ty): short sources whose footprint origin lies on its key grid."""
    f = flow[0].double().numpy()
    _, (fx, fy, ok) = key_counts(flow)
    short = (f[0] >= -RMAX) & (f[0] < RMAX - 1) & (f[1] >= -RMAX) & (f[1] < RMAX - 1)
    kx, ky = fx - tile[0] * TX + 1, fy - tile[1] * TY + 1
    return int((ok & short & (kx >= 0) & (kx <= TX) & (ky >= 0) & (ky <= TY)).sum())


def long_share(flow):
    f = flow[0].double().numpy()
    fin = np.isfinite(f).all(0)
    short = (f[0] >= -RMAX) & (f[0] < RMAX - 1) & (f[1] >= -RMAX) & (f[1] < RMAX - 1)
    return float((fin & ~short).mean())


def halo_variant(flow):
    """The widest halo variant (4, 8 or 16) some tile of the map takes: the reach of the short sources, as the pre-pass rounds it."""
    f = flow[0].double().numpy()
    short = np.isfinite(f).all(0) & (f[0] >= -RMAX) & (f[0] < RMAX - 1) & (f[1] >= -RMAX) & (f[1] < RMAX - 1)
    v = np.where(short, f, 0.0)
    r = np.where(v < 0, np.ceil(-v), np.floor(v) + 2).max()
    return 4 if r <= 4 else 8 if r <= 8 else 16


# ----------------------------------------------------------------------------------------- the kernels' host-visible rules, restated
# What splat_long_prepass / splat_tiled decide per source and per tile, from the fp32 splat flow [N, 2, H, W] alone (det_common.splat_flow
# for the DRM entry points).  Used to CHOOSE inputs and to ASSERT what a case reaches (tests/op_checks.py, the fused RIFE splats),
# never as a reference of values.
def _grid(h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return xs, ys


def tiles_of(h, w):
    """(tiles_y, tiles_x) of an h x w map"""
    return (h + TY - 1) // TY, (w + TX - 1) // TX


def source_class(flow):
    """-> (finite, short) [N, H, W] bool: splat_source_from's `finite` (the fp32 target x + f is finite) and `is_short`
    (f >= -RMAX and f < RMAX - 1 on both axes)."""
    flow = flow.float()
    xs, ys = _grid(*flow.shape[2:])
    finite = torch.isfinite(xs + flow[:, 0]) & torch.isfinite(ys + flow[:, 1])
    short = (flow[:, 0] >= -RMAX) & (flow[:, 0] < RMAX - 1) & (flow[:, 1] >= -RMAX) & (flow[:, 1] < RMAX - 1)
    return finite, short


def source_reach(flow, tight=0):
    """[N, H, W] int: the halo a finite short source asks for, as the pre-pass rounds it (f < 0: ceil(-f), else floor(f) + 2, the
    larger of the two axes); 0 for every other source.  tight=1, 2: floor(f) + 1 and floor(f), the roundings a later author may try."""
    flow = flow.float()
    finite, short = source_class(flow)
    r = torch.where(flow < 0, torch.ceil(-flow), torch.floor(flow) + (2 - int(tight)))
    r = torch.where((finite & short).unsqueeze(1).expand_as(r), r, torch.zeros_like(r))
    return torch.nan_to_num(r, 0.0, 0.0, 0.0).amax(1).long()


def tile_reach(flow, tight=0):
    """[N, tiles_y, tiles_x] int: the reach map, the max of source_reach over the sources of a 32 x 16 tile."""
    r = source_reach(flow, tight)
    n, h, w = r.shape
    ty, tx = tiles_of(h, w)
    pad = torch.zeros(n, ty * TY, tx * TX, dtype=r.dtype)
    pad[:, :h, :w] = r
    return pad.view(n, ty, TY, tx, TX).amax((2, 4))


def tile_variant(flow, use_map=None, tight=0, own_only=False):
    """[N, tiles_y, tiles_x] int in (4, 8, 16): the halo variant an output tile takes, the max of the reach map over its 3 x 3
    neighbourhood (inside the map), <= 4 -> 4, <= 8 -> 8, else 16; without the map (N * tiles > REACH_WORDS) every tile takes 16."""
    reach = tile_reach(flow, tight)
    n, ty, tx = reach.shape
    if use_map is None:
        use_map = n * ty * tx <= REACH_WORDS
    if not use_map:
        return torch.full_like(reach, RMAX)
    if not own_only:
        reach = torch.nn.functional.max_pool2d(reach[:, None].float(), 3, 1, 1)[:, 0].long()  # (reach >= 0: the padding never wins)
    return torch.where(reach <= 4, 4, torch.where(reach <= 8, 8, 16))


def record_keys(flow):
    """-> (kx, ky, is_record): the footprint origin floor(x + f) of every source as the fp32 sum gives it, and whether the tile
    kernel can hold the source as a record at all (finite and short)."""
    flow = flow.float()
    xs, ys = _grid(*flow.shape[2:])
    finite, short = source_class(flow)
    ok = finite & short
    kx = torch.where(ok, torch.floor(xs + flow[:, 0]), torch.full_like(flow[:, 0], -9.0)).long()
    ky = torch.where(ok, torch.floor(ys + flow[:, 1]), torch.full_like(flow[:, 1], -9.0)).long()
    return kx, ky, ok


def tile_record_totals(flow):
    """[N, tiles_y, tiles_x] int: the records of every output tile, the short sources whose footprint origin lies on the tile's
    33 x 17 key grid (-1 .. 31) x (-1 .. 15).  A source on a tile edge is a record of up to four tiles."""
    kx, ky, ok = record_keys(flow)
    n, h, w = ok.shape
    ty, tx = tiles_of(h, w)
    tot = torch.zeros(n, ty, tx, dtype=torch.long)
    item = torch.arange(n).view(n, 1, 1).expand(n, h, w)
    for dy in (0, 1):      # the tile of the footprint's lower right corner, and the tiles left of / above it that share the corner
        for dx in (0, 1):
            cx, cy = kx + dx, ky + dy
            # corner (cx, cy) names a tile; count the source once per distinct tile among its four corners
            first = ((dx == 0) | ((cx % TX) == 0)) & ((dy == 0) | ((cy % TY) == 0))
            m = ok & first & (cx >= 0) & (cy >= 0) & (cx // TX < tx) & (cy // TY < ty)
            # (a footprint origin at -1 has no tile of its own; one at tiles * 32 - 1 or beyond has none for its right corner)
            tot.index_put_((item[m], (cy // TY)[m], (cx // TX)[m]), torch.ones(int(m.sum()), dtype=torch.long), accumulate=True)
    return tot
