"""The DECISIONS of a GMFSS_UNION DRBA step, pixel by pixel.  (test infra)

The reference function has hard thresholds: the `cover < 0.999` hole tests of calc_drm_gmfss / calc_drm_rife_auxiliary
(oracle/drm.py `_fill`) and of Model.inference (`gaps0`, `gaps1`), and the `u / v > 25` swap masks at three pyramid scales
(oracle/gmfss.py GmfssModel.fusion_inputs).  Two evaluations that disagree on one of them differ by far more than rounding
after GridNet, so an end-to-end comparison has to forgive outliers -- and would forgive a wrong kernel with them.  This
module lets the tests compare the decisions themselves:

  * step_decisions(): the reference's boolean masks by name, from the two pair states of a step and its timesteps, with
    oracle.ops.softsplat on single-channel tensors; dtype-generic (fp32 = the oracle's arithmetic bit for bit, fp64);
  * unstable(): the same masks under six variants of the REFERENCE alone (fp32, fp64, four seeded one-ulp relative
    perturbations of the inputs): a pixel is unstable iff the six do not agree.  It uses nothing of the code under test;
  * Recorder: wraps drba_amd.ops.fill_holes / timestep_fix / swap_select for one step, recomputes each call's mask in torch
    with the kernel's own expression, and checks that recomputation against the kernel's output bit for bit;
  * compare(): HIP's mask == the reference's mask on the same pair state, everywhere except on unstable pixels, and the
    unstable set covers at most UNSTABLE_SHARE of a mask (a case with more tests nothing);
  * the row rules shared by the GPU checks and the planted-fault tests (tests/test_decisions.py): budget_ok (the old rule),
    flat rows, and two_branch_rows for the fused kernels whose hole test happens inside (flow_reverse, drm_rife_linear).
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle.ops import softsplat

HOLE = 0.999           # cover < HOLE: a hole (drm.py, GMFSS.py:116-117)
SWAP = 25              # u / v > SWAP: take the other side's pixel (GMFSS.py:125-150)
SCALES = (1.0, 0.5, 0.25)
ULP = 1.2e-7           # one ulp of an fp32 value, relative
SEEDS = (1, 2, 3, 4)
UNSTABLE_SHARE = 2e-4  # the suite's share for isolated decision flips: more unstable pixels than that and the case is useless
DRM_SITES = ("drm_fill_01", "drm_fill_12", "aux_fill_01", "aux_fill_12")
FUSION_SITES = ("gaps0", "gaps1") + tuple(f"swap_m{m}_s{s:g}" for s in SCALES for m in (0, 1))


# ----------------------------------------------------------------------------------------- the reference's decisions
def _distance(flow):
    """oracle.ops.distance without its cast to fp32 (it is what makes that function fp32-only)."""
    return torch.sqrt(flow[:, 0:1] ** 2 + flow[:, 1:] ** 2)


def _ratio_maps(flow10, flow12, eps):
    d10, d12 = _distance(flow10), _distance(flow12)
    if eps:
        d10, d12 = d10 + eps, d12 + eps
    return d10 / (d10 + d12), d12 / (d10 + d12)


def _retime(drm, t, linear, precision=1e-3):
    """drm * 2t, or oracle.drm.drm_to_t in the map's own dtype (the bisection of a scalar replayed on the map)."""
    if linear:
        return drm * t * 2
    x, frac, lo, hi = 0.5, 0.5, 0, 1
    xm, fm = drm.clone(), drm.clone()
    lom, him = xm * 0, xm * 0 + 1
    while abs(x - t) > precision:
        if x > t:
            hi = x
            x = x - (x - lo) * frac
            him = xm.clone()
            xm = xm - (xm - lom) * fm
        if x < t:
            lo = x
            x = x + (hi - x) * frac
            lom = xm.clone()
            xm = xm + (him - xm) * fm
    return xm


def drm_decisions(t, flow10, flow12, metric10, metric12, linear, values=False):
    """calc_drm_gmfss + calc_drm_rife_auxiliary (oracle/drm.py) with their hole masks brought out.
    -> (masks {drm_fill_01, drm_fill_12, aux_fill_01, aux_fill_12}, maps = calc_drm_gmfss' result, needed downstream;
    values=True adds calc_drm_rife_auxiliary's two maps to `maps`: two more splats, only the self-test wants them)."""
    drm10, drm12 = _ratio_maps(flow10, flow12, 0.0)
    d1t_01, d1t_12 = _retime(drm12, t, linear), _retime(drm10, t, linear)
    u01, u12 = 1 - d1t_01, 1 - d1t_12
    a01 = softsplat(u01, flow10, metric10, "soft")
    a12 = softsplat(u12, flow12, metric12, "soft")
    ones = a01 * 0 + 1
    masks = {"drm_fill_01": softsplat(ones, flow10, metric10, "soft") < HOLE,
             "drm_fill_12": softsplat(ones, flow12, metric12, "soft") < HOLE}
    maps = {"drm0t_t01": torch.where(masks["drm_fill_01"], u01, a01), "drm1t_t01": d1t_01,
            "drm1t_t12": d1t_12, "drm2t_t12": torch.where(masks["drm_fill_12"], u12, a12)}
    e10, e12 = _ratio_maps(flow10, flow12, 1e-4)
    u0, u1 = _retime(e10, t, linear), _retime(e12, t, linear)
    ones = e10 * 0 + 1
    masks["aux_fill_01"] = softsplat(ones, flow10 * u1, metric10, "soft") < HOLE
    masks["aux_fill_12"] = softsplat(ones, flow12 * u0, metric12, "soft") < HOLE
    if values:
        maps["drm_t1_t01"] = torch.where(masks["aux_fill_01"], u1, softsplat(u1, flow10 * u1, metric10, "soft"))
        maps["drm_t1_t12"] = torch.where(masks["aux_fill_12"], u0, softsplat(u0, flow12 * u0, metric12, "soft"))
    return masks, maps


def fusion_decisions(flow01, flow10, metric0, metric1, timestep0, timestep1):
    """The masks of GmfssModel.fusion_inputs with map timesteps: gaps0, gaps1, swap_m0_s{1,0.5,0.25}, swap_m1_s{...}."""
    F1t, F2t = timestep0 * flow01, timestep1 * flow10
    Z1t, Z2t = timestep0 * metric0, timestep1 * metric1
    t0 = softsplat(timestep0, F1t, Z1t, "soft")
    t1 = softsplat(timestep1, F2t, Z2t, "soft")
    masks = {"gaps0": softsplat(t0.clone() * 0 + 1, F1t, Z1t, "soft") < HOLE,
             "gaps1": softsplat(t1.clone() * 0 + 1, F2t, Z2t, "soft") < HOLE}
    bad = torch.logical_or(masks["gaps0"], masks["gaps1"])
    t0 = torch.where(bad, torch.ones_like(t0), t0)
    t1 = torch.where(bad, torch.ones_like(t1), t1)
    for s in SCALES:
        u, v = t0, t1
        if s != 1.0:
            u = F.interpolate(u, scale_factor=s, mode="bilinear", align_corners=False)
            v = F.interpolate(v, scale_factor=s, mode="bilinear", align_corners=False)
        masks[f"swap_m0_s{s:g}"] = u / v > SWAP
        masks[f"swap_m1_s{s:g}"] = v / u > SWAP
    return masks


def synthesised(ts):
    """The timesteps of a step that synthesise a frame, in output order (0, 1, 2 hand a source frame back)."""
    return [float(t) for t in ts if 0 < t < 1 or 1 < t < 2]


def step_decisions(ts, linear, flow10, flow01, metric1, metric0, flow12, flow21, metric1b, metric2):
    """Every mask of one inference_ts_drba step -> {"frame{k}/{site}": bool [1,1,h,w]}, k over the synthesised frames.
    The tensors are the first four entries of the step's two pair states: `reuse` (the (1,0) pair) and model.reuse(I1, I2)."""
    out, cache = {}, {}
    for k, t in enumerate(synthesised(ts)):
        left = t < 1
        tt = 1 - t if left else t - 1
        if tt not in cache:
            cache[tt] = drm_decisions(tt, flow10, flow12, metric1, metric1b, linear)
        dm, dg = cache[tt]
        fm = (fusion_decisions(flow10, flow01, metric1, metric0, dg["drm1t_t01"], dg["drm0t_t01"]) if left else
              fusion_decisions(flow12, flow21, metric1b, metric2, dg["drm1t_t12"], dg["drm2t_t12"]))
        for name, m in list(dm.items()) + list(fm.items()):
            out[f"frame{k}/{name}"] = m
    return out


def reference_decisions(r10, r12, ts, linear):
    """step_decisions on two pair states as the models carry them (flow, flow, metric, metric, features, features), fp32."""
    return step_decisions(ts, linear, *[t.detach().float().cpu() for t in list(r10[:4]) + list(r12[:4])])


# ----------------------------------------------------------------------------------------- which pixels are undecided
def variants(inputs, seeds=SEEDS, rel=ULP):
    """[(name, inputs')]: fp32 as given, fp64, and per seed a relative perturbation of +-rel of every element (None stays None)."""
    cast = lambda f: [None if t is None else f(t) for t in inputs]  # noqa: E731
    out = [("fp32", cast(lambda t: t.float())), ("fp64", cast(lambda t: t.double()))]
    for seed in seeds:
        g = torch.Generator().manual_seed(seed)
        out.append((f"seed{seed}", cast(lambda t: t.float() * (1 + rel * (torch.randint(0, 2, t.shape, generator=g) * 2 - 1).float()))))
    return out


def disagreement(runs):
    """runs: one {site: bool mask} per variant -> {site: mask of the pixels on which the variants do not ALL agree}.
    Symmetric in the order of the runs."""
    out = {}
    for site in runs[0]:
        stack = torch.stack([r[site] for r in runs])
        out[site] = ~(stack.all(0) | (~stack).all(0))
    return out


def unstable(fn, inputs, seeds=SEEDS, rel=ULP):
    """fn(*inputs) -> {site: mask}, evaluated under variants(): -> (the fp32 masks, {site: unstable pixels})."""
    runs = [fn(*v) for _, v in variants(inputs, seeds, rel)]
    return runs[0], disagreement(runs)


def step_unstable(r10, r12, ts, linear, seeds=SEEDS):
    """reference_decisions and their unstable sets for one step."""
    ins = [t.detach().float().cpu() for t in list(r10[:4]) + list(r12[:4])]
    return unstable(lambda *a: step_decisions(ts, linear, *a), ins, seeds)


def hole_unstable(flow, seeds=SEEDS):
    """The hole test of the fused RIFE kernels (flow_reverse, drm_rife_linear): ones-splat along `flow`, mode avg, < 0.999.
    -> (mask, unstable), both [N,1,H,W]."""
    m, u = unstable(lambda f: {"hole": softsplat(torch.ones_like(f[:, :1]), f, None, "avg") < HOLE}, [flow], seeds)
    return m["hole"], u["hole"]


# ----------------------------------------------------------------------------------------- the code under test's decisions
def _same(a, b):
    """Number of elements that are not equal bit for bit (NaN positions must coincide)."""
    ok = (a == b) | (a.isnan() & b.isnan())
    return int((~ok).sum())


class Recorder:
    """Wraps ops.fill_holes / timestep_fix / swap_select (the model code looks them up as _ops.<name> at call time).  Per call:
    the mask recomputed in torch on the device with the kernel's own expression, and how many elements of the kernel's output
    differ from the selection that mask implies (0: the recomputed mask IS the kernel's decision)."""
    NAMES = ("fill_holes", "timestep_fix", "swap_select")

    def __init__(self, ops):
        self.ops = ops
        self.fills, self.fixes, self.swaps = [], [], []  # [(masks..., differing elements)]

    def __enter__(self):
        self._orig = {n: getattr(self.ops, n) for n in self.NAMES}
        orig = self._orig

        def fill_holes(aligned, cover, value):
            out = orig["fill_holes"](aligned, cover, value)
            mask = cover < HOLE
            self.fills.append((mask.cpu(), _same(out, torch.where(mask, value, aligned))))
            return out

        def timestep_fix(t0, t1, cover0, cover1):
            o0, o1 = orig["timestep_fix"](t0, t1, cover0, cover1)
            g0, g1 = cover0 < HOLE, cover1 < HOLE
            bad = g0 | g1
            diff = _same(o0, torch.where(bad, torch.ones_like(t0), t0)) + _same(o1, torch.where(bad, torch.ones_like(t1), t1))
            self.fixes.append((g0.cpu(), g1.cpu(), diff))
            return o0, o1

        def swap_select(x, y, t0, t1, thr=25.0, out=None):
            x0, y0 = x.clone(), y.clone()  # (in place the kernel overwrites its inputs)
            ox, oy = orig["swap_select"](x, y, t0, t1, thr, out=out)
            m0, m1 = (t0 / t1) > thr, (t1 / t0) > thr
            diff = _same(ox, torch.where(m0, y0, x0)) + _same(oy, torch.where(m1, x0, y0))
            self.swaps.append((m0.cpu(), m1.cpu(), diff))
            return ox, oy

        for n, f in (("fill_holes", fill_holes), ("timestep_fix", timestep_fix), ("swap_select", swap_select)):
            setattr(self.ops, n, f)
        return self

    def __exit__(self, *exc):
        for n, f in self._orig.items():
            setattr(self.ops, n, f)
        return False

    def masks(self, n_frames):
        """-> ({"frame{k}/{site}": mask}, rows of the bit-exact recomputation).  A step makes, per synthesised frame, four
        fill_holes (calc_drm_gmfss 01, 12; calc_drm_rife_auxiliary 01, 12), then one timestep_fix and four swap_select (the
        half-resolution frames and the pyramid levels at scales 1, 0.5, 0.25); another call pattern is an error here."""
        got = (len(self.fills), len(self.fixes), len(self.swaps))
        assert got == (4 * n_frames, n_frames, 4 * n_frames), f"fill_holes / timestep_fix / swap_select calls {got} for {n_frames} frames"
        out = {}
        for k in range(n_frames):
            for j, site in enumerate(DRM_SITES):
                out[f"frame{k}/{site}"] = self.fills[4 * k + j][0]
            out[f"frame{k}/gaps0"], out[f"frame{k}/gaps1"] = self.fixes[k][:2]
            for j, s in enumerate((1.0, 1.0, 0.5, 0.25)):  # (frames and level 1 share the full-size masks)
                m0, m1, _ = self.swaps[4 * k + j]
                if j == 1:
                    assert torch.equal(m0, out[f"frame{k}/swap_m0_s1"]) and torch.equal(m1, out[f"frame{k}/swap_m1_s1"])
                out[f"frame{k}/swap_m0_s{s:g}"], out[f"frame{k}/swap_m1_s{s:g}"] = m0, m1
        px = lambda calls: sum(c[0].numel() for c in calls)  # noqa: E731
        rows = [(f"{name}: kernel output vs torch.where on the recomputed mask, differing elements", float(sum(c[-1] for c in calls)), 0.0,
                 f"{len(calls)} calls, {px(calls)} mask pixels")
                for name, calls in (("fill_holes", self.fills), ("timestep_fix", self.fixes), ("swap_select", self.swaps))]
        return out, rows


@contextlib.contextmanager
def oracle_pair_state(ora, r12):
    """For the duration: GmfssUnionOracle's model.reuse returns `r12` -- inference_ts_drba(..., reuse=r10) then runs the
    reference's step on two GIVEN pair states (everything downstream of them is the oracle's arithmetic)."""
    ora.model.reuse = lambda *a, **k: r12
    try:
        yield ora
    finally:
        del ora.model.reuse  # (the instance attribute: the class's method is back)


# ----------------------------------------------------------------------------------------- row rules
def budget_ok(d, n_out, n):
    """The outlier budget of the end-to-end GMFSS_UNION rows: at most n // 5000 elements above the tolerance, none above 5e-2."""
    return n_out <= n // 5000 and d <= 5e-2


def compare(hip, ref, unst, label=""):
    """Rows per decision site: HIP's mask must equal the reference's on every stable pixel (mismatches there: 0), and the
    unstable set may cover at most UNSTABLE_SHARE of the mask.  Details: mismatches / unstable / pixels."""
    assert set(hip) == set(ref) == set(unst), (sorted(hip), sorted(ref))
    rows = []
    for site in ref:
        h, r, u = hip[site].cpu(), ref[site], unst[site]
        assert h.shape == r.shape == u.shape, (site, h.shape, r.shape)
        mism = h != r
        n = r.numel()
        rows.append((f"{label}decision {site}: mismatches on stable pixels", float(int((mism & ~u).sum())), 0.0,
                     f"mismatches / unstable / pixels = {int(mism.sum())} / {int(u.sum())} / {n}, set {int(r.sum())}"))
        rows.append((f"{label}decision {site}: unstable share", int(u.sum()) / n, UNSTABLE_SHARE, ""))
    return rows


def two_branch_rows(name, got, aligned, fill, hole, unst, tol, fill_mask_of=None):
    """A fused kernel whose hole test happens inside (no mask comes out), against the reference's two branches:
    outside `unst` the value is flat within tol of the reference's choice; on an unstable pixel it must be, to the same
    tolerance, ONE of the two branches (`aligned` or `fill`).  fill_mask_of(got) -> the kernel's decision where its output
    lets it be read (then it must equal `hole` outside `unst`).  All tensors broadcast against `got`; NaNs must coincide."""
    got, aligned, fill = got.detach().float().cpu(), aligned.float(), fill.float()
    hole, unst = hole.expand_as(got), unst.expand_as(got)
    fill, aligned = fill.expand_as(got), aligned.expand_as(got)

    def err(a, b):
        nan_ok = a.isnan() == b.isnan()
        d = (torch.nan_to_num(a, nan=0.0, posinf=3e38, neginf=-3e38) - torch.nan_to_num(b, nan=0.0, posinf=3e38, neginf=-3e38)).abs()
        return torch.where(nan_ok, d, torch.full_like(d, float("inf")))

    e_ref = err(got, torch.where(hole, fill, aligned))
    e_either = torch.minimum(err(got, aligned), err(got, fill))
    stable = ~unst
    rows = [(f"{name}: stable pixels", float(e_ref[stable].max()) if bool(stable.any()) else 0.0, tol,
             f"unstable {int(unst.sum())}/{unst.numel()}"),
            (f"{name}: unstable pixels, nearer branch", float(e_either[unst].max()) if bool(unst.any()) else 0.0, tol, ""),
            (f"{name}: unstable share", int(unst.sum()) / unst.numel(), UNSTABLE_SHARE, "")]
    if fill_mask_of is not None:
        bad = (fill_mask_of(got) != hole) & stable
        rows.append((f"{name}: hole mask read from the output, mismatches on stable pixels", float(int(bad.sum())), 0.0, f"holes {int(hole.sum())}"))
    return rows
