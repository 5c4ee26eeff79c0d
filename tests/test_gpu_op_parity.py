"""GPU (-m gpu): every pointwise / gather / reduction kernel of the GMFlow and GMFSS glue, the generic forward splat
(count, scan, fill, gathers), resize_bilinear_scale, flow_distance and the IFNet stage glue (stage-input gathers, the gathers
fused with conv0[0], flow update, final warp + blend: [H,W,4] frames, pair-only features, the flow as terms, the blend at the
frame's own resolution) on their own against a float64 reference (tests/op_checks.py), at the sizes where kernels go wrong:
image borders, partial tiles and blocks, every dispatch branch, batch > 1, grid-stride loops and scan rounds that go round
twice.  One operator family per test, so that a failure names it.  The 3x3 convolution's epilogue forms (op_checks.CONV_FORMS: what
the GMFlow / GMFSS layers construct) run with every configuration id pinned, one test per kernel family and form group.  The fused
window attention, the global expectation and the split linear layer run at every edge of their host dispatch (key runs, wave forms,
token table, tile forms), with the form that ran read from the kernel trace and sentinels behind outputs and workspaces.  IFNet's
context encoder as one kernel runs in both of its forms (head_fused.hip, head_fused16.hip) at every tile, border and store edge
(op_checks.HEAD_CASES), on zero, signed and NaN-pixel frames, as a batch through the C ABI into guarded outputs, at its refusals and at
the shapes that fall back to the layer chain.  The fused RIFE splats (splat_long_prepass / splat_tiled and the _det pair) run on
sources planted at the window edges of every halo variant, at the reach roundings, next to quiet tiles, at the record capacity, on
maps smaller than a tile, with non-finite and far flows, as 8 items, and in launches too large for the reach map.

Value rows: tol = max(2e-5 max(1, |ref|max), 3 x the fp32 oracle's own error on that input); decisions and data movement:
bit-exact.  tests/test_op_checks_cpu.py shows on the CPU that these rows fail for a wrong operator."""
import pytest
import torch

from tests import op_checks, report

pytestmark = pytest.mark.gpu


def _assert_rows(rows):
    import inspect
    report.record(inspect.stack()[1].function, rows)
    for n, e, t, x in rows:
        print(f"  {n:58s} err={e:.3e} tol={t:.1e} {x}")
    bad = [(n, e, t, x) for n, e, t, x in rows if not e <= t]
    assert not bad, "\n".join(f"{n}: err={e:.3e} tol={t:.1e} {x}" for n, e, t, x in bad)


def test_softmax_rows(hip_backend):
    _assert_rows(op_checks.check_softmax_rows(hip_backend.dev))


def test_instance_norm(hip_backend):
    _assert_rows(op_checks.check_instance_norm(hip_backend.dev))


def test_conv_direct(hip_backend):
    _assert_rows(op_checks.check_conv_direct(hip_backend.dev))


def test_local_corr_flow(hip_backend):
    _assert_rows(op_checks.check_local_corr_flow(hip_backend.dev))


def test_local_attn_flow(hip_backend):
    _assert_rows(op_checks.check_local_attn_flow(hip_backend.dev))


def test_convex_upsample(hip_backend):
    _assert_rows(op_checks.check_convex_upsample(hip_backend.dev))


def test_flow_warp(hip_backend):
    _assert_rows(op_checks.check_flow_warp(hip_backend.dev))


def test_backwarp(hip_backend):
    _assert_rows(op_checks.check_backwarp(hip_backend.dev))


def test_resize_bilinear_ac(hip_backend):
    _assert_rows(op_checks.check_resize_bilinear_ac(hip_backend.dev))


def test_layernorm(hip_backend):
    _assert_rows(op_checks.check_layernorm(hip_backend.dev))


def test_gelu(hip_backend):
    _assert_rows(op_checks.check_gelu(hip_backend.dev))


def test_bmm(hip_backend):
    _assert_rows(op_checks.check_bmm(hip_backend.dev))


def test_pointwise(hip_backend):
    _assert_rows(op_checks.check_pointwise(hip_backend.dev))


def test_layouts(hip_backend):
    _assert_rows(op_checks.check_layouts(hip_backend.dev))


def test_hole_tests(hip_backend):
    _assert_rows(op_checks.check_hole_tests(hip_backend.dev))


def test_drm_ratio_and_retime(hip_backend):
    _assert_rows(op_checks.check_drm(hip_backend.dev))


def test_metric_input(hip_backend):
    _assert_rows(op_checks.check_metric_input(hip_backend.dev))


SCAN_PER_BLOCK = 4096         # kScanPerBlock, drba_amd/csrc/splat_warp.hip:668 (keys per scan_block workgroup), restated
SCAN_SUMS_ROUND = 256         # block sums scan_sums takes per round of its carry loop, splat_warp.hip:734 (b0 += 256)
GRID_STRIDE = 2048 * 256      # kMaxBlocks x kBlock, drba_amd/csrc/common.hpp:92-96 (grid_for): pixels one round of a grid-stride loop covers


def _scan_blocks(n, h, w):
    return -(-op_checks.splat_keys(n, h, w) // SCAN_PER_BLOCK)


def test_softsplat(hip_backend):
    _assert_rows(op_checks.check_softsplat(hip_backend.dev))


def test_softsplat_scan_geometry(hip_backend):
    """One full scan block, two, a ragged second one, image boundaries inside a block -- asserted from the restated constant, so
    that a change of kScanPerBlock fails here instead of silently un-covering the multi-block scan."""
    assert [op_checks.splat_keys(*c) for c in op_checks.SCAN_CASES[:3]] == [SCAN_PER_BLOCK, 2 * SCAN_PER_BLOCK, SCAN_PER_BLOCK + 64]
    assert [_scan_blocks(*c) for c in op_checks.SCAN_CASES] == [1, 2, 2, 4, 3]
    for n, h, w in op_checks.SCAN_CASES[3:]:  # N = 3: no image starts on a block boundary, and some block holds keys of two images
        starts = [k * (h + 1) * (w + 1) for k in (1, 2)]
        assert all(s % SCAN_PER_BLOCK for s in starts) and starts[0] // SCAN_PER_BLOCK < _scan_blocks(n, h, w) - 1
    rows = op_checks.check_softsplat_scan(hip_backend.dev)
    assert all(f"keys={op_checks.splat_keys(*c)}" in " ".join(r[3] for r in rows) for c in op_checks.SCAN_CASES)
    _assert_rows(rows)


def test_softsplat_big_map(hip_backend):
    """scan_sums goes round its carry loop more than once (nb > 256, dozens of blocks in the second round) and the grid-stride
    loops of splat_sort_count / splat_sort_fill more than twice: code that no smaller map of the suite runs."""
    h, w = op_checks.SPLAT_BIG
    nb = _scan_blocks(1, h, w)
    assert nb > SCAN_SUMS_ROUND + 32 and op_checks.splat_keys(1, h, w) > 1_200_000  # splat_warp.hip:668, 734
    assert h * w > 2 * GRID_STRIDE                                                 # common.hpp:92-96
    _assert_rows(op_checks.check_softsplat_big(hip_backend.dev))


def test_resize_bilinear_scale(hip_backend):
    _assert_rows(op_checks.check_resize_scale(hip_backend.dev))


def test_flow_distance(hip_backend):
    _assert_rows(op_checks.check_flow_distance(hip_backend.dev))


# ----------------------------------------------------------------------------------------- the IFNet stage glue
def test_stage_input_first(hip_backend):
    _assert_rows(op_checks.check_stage_input_first(hip_backend.dev))


def test_stage_input_warped(hip_backend):
    _assert_rows(op_checks.check_stage_input_warped(hip_backend.dev))


def test_stage_conv_fused(hip_backend):
    _assert_rows(op_checks.check_stage_conv_fused(hip_backend.dev))


def test_flow_update(hip_backend):
    _assert_rows(op_checks.check_flow_update(hip_backend.dev))


def test_warp_blend(hip_backend):
    _assert_rows(op_checks.check_warp_blend(hip_backend.dev))


def _traced(fn):
    """fn() -> (its result, the kernel names launched inside it)"""
    from drba_amd import ops
    torch.cuda.synchronize()
    ops.trace_begin()
    try:
        got = fn()
        torch.cuda.synchronize()
    finally:
        recs = ops.trace_end()
    return got, [r["name"] for r in recs]


B_ = {True: "true", False: "false"}
GLUE_FORMS = (  # regular expressions over the kernel names, template arguments as tests/golden/ops_launches.json shows them
    [rf"ifblock_input_lds<{B_[sg]}, ?{fm}, ?{B_[vs]}>" for sg in (True, False) for fm in (0, 1, 2) for vs in (True, False)]
    + [rf"ifblock_input_pixel<{B_[hf]}, ?true>" for hf in (True, False)]
    + [rf"ifblock_input_kernel<{B_[hf]}, ?false, ?1>" for hf in (True, False)]
    + [r"warp_blend_fold_kernel<true, ?true>", r"warp_blend_fold_kernel<true>|warp_blend_fold_kernel<true, ?false>",
       r"warp_blend_fold_kernel<false>|warp_blend_fold_kernel<false, ?false>", r"warp_blend_kernel", r"ifblock_update_kernel",
       r"stage_conv16<", r"stage_conv16_s2<.*Geo<\d+, ?1>", r"stage_conv16_s2<.*Geo<\d+, ?2>"]
    + [rf"stage_conv0<{fm}," for fm in (0, 1, 2)])


def test_glue_rows_run_the_branches_they_name(hip_backend):
    """The five glue checks again under the kernel trace: every form of the stage-input gathers (one sample point or four, flow
    finished / folded / as terms, vector or scalar stores), the first stage's two kernels with and without a flow, the three
    blends, both fused convolutions at scale 1 and the scale-2 one with one and two n-tiles were launched at least once -- a
    later change of a tile size or a dispatch rule that un-covers a form fails here instead of passing quietly."""
    import re
    _, names = _traced(lambda: [check(hip_backend.dev) for check in op_checks.GLUE_CHECKS])
    seen = sorted(set(names))
    print("  launched:\n    " + "\n    ".join(seen))
    missing = [f for f in GLUE_FORMS if not any(re.search(f, n) for n in seen)]
    assert not missing, f"never launched: {missing}\nlaunched: {seen}"


def test_layout_copies_are_what_is_read(hip_backend):
    """Which layout a gather reads is a run-time pointer, invisible in the trace.  The copy ops.rgbx / ops.pair_interleaved
    returns is scaled by 2 in place (the frame's own version does not move, so the copy stays current): where the copy is read,
    the frame (feature) channels double exactly and nothing else moves; at scale 4 stage_inputs hands no copies over and the
    result is the same bit for bit."""
    from drba_amd import ops
    dev = hip_backend.dev
    h, w = 64, 128
    fr = op_checks.glue_frames(1, h, w, 4000)
    heads = op_checks.glue_heads(1, h, w, (16, 8, 4, 2, 1), 4010)
    D = lambda t: t.to(dev)  # noqa: E731
    flow = D(op_checks.flows4(h, w, 4020)["smooth"])
    wt, bs = op_checks.cases.rnd((16, 52, 3, 3), 4030, 1.0 / (52 * 9) ** 0.5), op_checks.cases.rnd((16,), 4031, 0.1)
    conv = ops.Conv3x3(wt, bs, 2, True, None, device=dev)

    def stage(it, s):
        return op_checks._stage_inputs_out(ops, dev, [it], [flow], D(heads[2 * s]), 2 * s, s)[0]

    def blend(it, last, tscales):
        return ops.warp_blend_lazy([it[:2]], [(D(heads[t]), float(t)) for t in tscales], D(heads[last]), float(last))[0]

    runs = {"ifblock_input_lds s=1": lambda it: stage(it, 1), "ifblock_input_lds s=2": lambda it: stage(it, 2),
            "ifblock_input_lds s=4": lambda it: stage(it, 4), "stage_conv0 s=1": lambda it: ops.stage_conv0([it], [flow], D(heads[2]), 2.0, conv)[0],
            "warp_blend_lazy S1": lambda it: blend(it, 1, (8, 4, 2)), "warp_blend_lazy staged": lambda it: blend(it, 2, (16, 8, 4))}
    for name, run in runs.items():
        it = op_checks.glue_item(dev, ops, fr, 0, x4=True)
        before = run(it).clone()
        for img in it[:2]:
            v = img._version
            ops.rgbx(img).mul_(2.0)
            assert img._version == v and ops._x4_of(img) is not None
        after = run(it)
        torch.cuda.synchronize()
        assert float(before.abs().max()) > 0 and torch.isfinite(before).all()
        if name.endswith("s=4"):
            assert torch.equal(after, before), f"{name}: the [H,W,4] copies are read"
        elif name.startswith("stage_conv0"):
            assert not torch.equal(after, before), f"{name}: the [H,W,4] copies are not read"
        elif name.startswith("warp_blend"):
            assert torch.equal(after, 2.0 * before), f"{name}: the [H,W,4] copies are not what is read"
        else:
            assert torch.equal(after[:, :6], 2.0 * before[:, :6]) and torch.equal(after[:, 6:], before[:, 6:]), f"{name}: the [H,W,4] copies are not what is read"
    for s in (4, 1):  # the first stage: ifblock_input_kernel / ifblock_input_pixel <false, ...> on pair-only features
        it = op_checks.glue_item(dev, ops, fr, 0, pair=True)
        assert ops.is_pair(it[3]) and ops.is_pair(it[4])
        before = ops.ifblock_input(it[0], it[1], it[3], it[4], it[2], None, None, 1.0, float(s)).clone()
        it[3].mul_(2.0), it[4].mul_(2.0)
        after = ops.ifblock_input(it[0], it[1], it[3], it[4], it[2], None, None, 1.0, float(s))
        assert torch.equal(after[:, 6:38], 2.0 * before[:, 6:38]) and torch.equal(after[:, :6], before[:, :6]) and torch.equal(after[:, 38:], before[:, 38:])
    torch.cuda.synchronize()


WS_GUARD = 4096
WS_SHAPES = ((1, 1, 1), (1, 2, 2), (1, 1, 2), (1, 2, 4),  # (N, H, W): L = N (H + 1) (W + 1) = 4, 9, 6, 15 -- every residue mod 4, one block
             (1, 63, 64), (1, 90, 90), (2, 78, 80), (1, 128, 130))  # 4160 (2 blocks), 8281 (3), 12798 (4), 16899 (5): residues 0, 1, 2, 3


def test_softsplat_workspace_guard(hip_backend):
    """drba_softsplat on a workspace of exactly drba_softsplat_ws_floats(N, C, H, W) floats followed by 4096 sentinel floats (one
    allocation: nothing is written outside allocated memory whatever the layout does): the sentinels are untouched and the
    output holds its fp64 row, for every residue of the key count mod 4 (the alignment padding of start / bsum / rec in
    splat_ws), 1 to 5 scan blocks, a quad-gather and a planar-gather channel count each."""
    import ctypes as C
    from drba_amd import _lib, ops
    lib, dev = _lib.load(), hip_backend.dev
    keys = [op_checks.splat_keys(*s) for s in WS_SHAPES]
    assert {k % 4 for k in keys} == {0, 1, 2, 3} and {-(-k // SCAN_PER_BLOCK) for k in keys} == {1, 2, 3, 4, 5}
    assert {k % 4 for k in keys[:4]} == {0, 1, 2, 3} == {k % 4 for k in keys[4:]}
    rows = []
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for i, (n, h, w) in enumerate(WS_SHAPES):
        for c in (16, 3):
            mode = op_checks.SPLAT_MODES[(i + c) % 4]
            x, flow, metric = op_checks.splat_inputs(n, c, h, w, 2700 + 3 * i, mode, sigma=1.5)
            size = lib.drba_softsplat_ws_floats(n, c, h, w)
            ws = torch.full((size + WS_GUARD,), 1.2345e-3, device=dev)
            out = torch.full((n, c, h, w), float("nan"), device=dev)
            xd, fd, md = x.to(dev), flow.to(dev), None if metric is None else metric.to(dev)
            rc = lib.drba_softsplat(ptr(xd), ptr(fd), C.c_void_p(0) if md is None else ptr(md), ptr(out), ptr(ws), n, c, h, w, ops._MODES[mode], 0,
                                    ops._stream())
            assert rc == 0, (rc, n, c, h, w)
            name = f"{mode} ws guard N={n} C={c} {h}x{w}"
            rows.append(op_checks.value_row("softsplat", name, out, *op_checks.splat_refs(name, x, flow, metric, mode),
                                            f"keys={keys[i]} ws={size} floats"))
            rows.append(op_checks.exact_row("softsplat", f"{name}: the {WS_GUARD} floats behind the workspace", ws[size:],
                                            torch.full((WS_GUARD,), 1.2345e-3)))
    _assert_rows(rows)


def test_softsplat_reuse_index_launches_one_gather(hip_backend):
    """check_softsplat's reuse_index=True row again, with the kernel trace on: the values are the same whether the index was
    reused or quietly rebuilt, the launches are not.  A reused index is one gather launch and nothing of count / scan / fill;
    after an in-place update of the flow the same call has to rebuild (ops.softsplat_many drops its token), and the trace shows
    that too -- so the first assertion is not one that any call would pass."""
    from drba_amd import ops
    dev = hip_backend.dev
    xs, flow, metric = op_checks.many_inputs()
    fd, md, x17 = flow.to(dev), metric.to(dev), xs[2].to(dev)

    def traced():
        torch.cuda.synchronize()
        ops.trace_begin()
        try:
            got = ops.softsplat_many([x17], fd, md, "soft", reuse_index=True)[0]
            torch.cuda.synchronize()
        finally:
            recs = ops.trace_end()
        return got, [r["name"] for r in recs]

    ops.softsplat_many([x.to(dev) for x in xs], fd, md, "soft")
    got, names = traced()
    print(f"  reuse_index=True launches: {names}")
    assert len(names) == 1 and "splat_sorted_gather" in names[0], names
    rows = [op_checks.value_row("softsplat", op_checks.REUSE_ROW, got, *op_checks.splat_refs(op_checks.REUSE_ROW, xs[2], flow, metric, "soft"))]
    fd.add_(0.0)  # same values, a new version: the index on record is no longer vouched for
    got, names = traced()
    print(f"  reuse_index=True after an in-place update of the flow: {names}")
    assert any("splat_sort_count" in n for n in names) and any("splat_sort_fill" in n for n in names), names
    rows.append(op_checks.value_row("softsplat", op_checks.REUSE_ROW + ", flow updated in place: rebuilt", got,
                                    *op_checks.splat_refs(op_checks.REUSE_ROW, xs[2], flow, metric, "soft")))
    _assert_rows(rows)


# ----------------------------------------------------------------------------------------- the convolution epilogue forms
def _conv_ids(family):
    lib = op_checks.conv_lib()
    return lib, [c for c in range(lib.drba_conv3x3_num_cfgs()) if lib.drba_conv3x3_cfg_family(c) == family]


@pytest.mark.parametrize("group", ("plain", "residual"))
@pytest.mark.parametrize("family", (0, 1, 2, 3, 4))
def test_conv_forms(hip_backend, family, group):
    """Every id of the family, pinned, in every form of the group that applies to its stride (op_checks.CONV_FORMS), on the two
    guarded maps and the tiny ones: value rows against fp64, sentinel rows around out=.  Completeness: every (id, form) that applies
    has an accepted launch; the only refusals are the documented ones (W % 4 != 0 on the LDS-DMA members)."""
    lib, ids = _conv_ids(family)
    forms = op_checks.CONV_PLAIN_FORMS if group == "plain" else op_checks.CONV_RESIDUAL_FORMS
    rows = op_checks.check_conv_forms(hip_backend.dev, cfgs=ids, forms=forms)
    torch.cuda.synchronize()
    print(f"  refused (documented): {sorted(set(op_checks.CONV_REFUSED))}")
    assert all(op_checks.conv_id_class(lib, c) == "dma" and int(what.split("x")[2]) % 4 for c, what in op_checks.CONV_REFUSED)
    missing = op_checks.conv_forms_missing(rows, lib, ids, forms)
    assert not missing, f"no accepted row for (id, form): {missing}"
    _assert_rows(rows)


def test_conv_forms_cover_every_id():
    """the five families of test_conv_forms are all 38 ids, the two groups all 12 forms"""
    assert sorted(c for f in range(5) for c in _conv_ids(f)[1]) == list(range(38))
    assert set(op_checks.CONV_PLAIN_FORMS) | set(op_checks.CONV_RESIDUAL_FORMS) == {f.name for f in op_checks.CONV_FORMS}
    assert len(op_checks.CONV_FORMS) == 12


def test_conv_relu_on_a_non_finite_sum(hip_backend):
    """bias + ReLU with a NaN in the input and -inf as one channel's bias, every id, both store paths: the NaN stays, -inf gives +0"""
    rows = op_checks.check_conv_relu_nonfinite(hip_backend.dev)
    assert {r.cfg for r in rows if r.kind == "nonfinite"} == set(range(38))
    _assert_rows(rows)


def test_deconv_and_shuffle_store_guards(hip_backend):
    """Deconv4x4 (all 15 ids, with and without PixelShuffle) and conv3x3 + PixelShuffle with act="prelu" into guarded outputs"""
    rows = op_checks.check_deconv_guard(hip_backend.dev)
    for ps in (0, 1):
        assert {r.cfg for r in rows if r.kind == "guard" and f"ps={ps}" in r[0]} == set(range(15))
    _assert_rows(rows + op_checks.check_shuffle_guard(hip_backend.dev))


def _traced_recs(fn):
    from drba_amd import ops
    torch.cuda.synchronize()
    ops.trace_begin()
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        recs = ops.trace_end()
    return recs


RL_KERNELS = {  # kernel -> its name with the RL template argument true, as the trace records it
    "conv_split_mfma": r"conv_split_mfma<.*SplitCfg<[^>]*>, ?(true|false), ?true",
    "conv_dma1": r"conv_dma1<(true|false), ?true",
    "conv_ks": r"conv_ks<\d+, ?(true|false), ?true"}


def test_same_tensor_resconv_rows_run_rl_kernels(hip_backend):
    """The ResConv rows whose residual IS the input tensor launch the "residual from LDS" instantiation of conv_split_mfma, conv_dma1
    and conv_ks at least once each; the rows with a second copy of the input launch none.  Read from the kernel names and template
    arguments of the trace: a change of the launchers' res == in rule that un-covers RL fails here."""
    import re
    lib = op_checks.conv_lib()
    ids = [c for c in range(lib.drba_conv3x3_num_cfgs()) if op_checks.conv_id_class(lib, c) in ("split", "dma", "ks")]
    names, rows = {}, []
    for form in ("resconv res is in", "resconv res copy"):
        recs = _traced_recs(lambda: rows.extend(op_checks.check_conv_forms(hip_backend.dev, cfgs=ids, forms=(form,))))
        names[form] = sorted({r["name"] for r in recs if "conv_" in r["name"]})
        print(f"  {form}:\n    " + "\n    ".join(names[form]))
    for kernel, rl in RL_KERNELS.items():
        assert any(kernel in n for n in names["resconv res copy"]), (kernel, names["resconv res copy"])
        assert any(re.search(rl, n) for n in names["resconv res is in"]), f"no RL instantiation of {kernel}: {names['resconv res is in']}"
        assert not any(re.search(rl, n) for n in names["resconv res copy"]), f"RL {kernel} on a second copy: {names['resconv res copy']}"
    _assert_rows(rows)


def test_conv_many_items(hip_backend):
    """A batch of 128 small maps, 32 -> 32, in the two forms the 1080p rows do not cover, on every stride-1 id that accepts the
    layer.  That the batch is large enough for the persistent loops is read from the traced grid, not from restated tile sizes:
    for every id of families 1 and 2 and their family-4 members the grid at N equals the grid at N / 2, so those workgroups take at
    least two tiles each.  (fp32 and K-split grids grow with the batch: value rows only.)"""
    from drba_amd import ops
    dev = hip_backend.dev
    lib = op_checks.conv_lib()
    rows = op_checks.check_conv_many(dev)
    ids = op_checks.conv_many_ids(lib)
    assert {(r.cfg, r.form) for r in rows if r.kind == "value"} == {(c, f) for c in ids for f in op_checks.MANY_FORMS}
    persistent = [c for c in ids if op_checks.conv_id_class(lib, c) in ("split", "dma")]
    assert {lib.drba_conv3x3_cfg_family(c) for c in persistent} == {1, 2, 4} and len(persistent) >= 8
    n = op_checks.MANY_N
    for form in (f for f in op_checks.CONV_FORMS if f.name in op_checks.MANY_FORMS):
        d = op_checks.conv_many_inputs(dev, form)
        for cfg in persistent:
            layer, _ = op_checks.conv_many_layer(ops, dev, form, cfg)
            grids = []
            for m in (n, n // 2):
                x = d["x"][:m]
                res, res2 = (x, None) if form.res == "same" else (d["res"][:m], d["res2"][:m])
                recs = [r for r in _traced_recs(lambda: layer(x, residual=res, residual2=res2)) if "conv_" in r["name"]]
                assert len(recs) == 1, recs
                grids.append(recs[0]["grid"])
            print(f"  cfg{cfg} {form.name}: grid {grids[0]} at N={n}, {grids[1]} at N={n // 2} ({recs[0]['name']})")
            assert grids[0] == grids[1], f"cfg{cfg} {form.name}: the grid still grows with the batch ({grids[1]} -> {grids[0]}): N = {n} is too small"
    _assert_rows(rows)


def test_documented_refusals(hip_backend):
    """Shapes a launcher documents as refused raise DrbaHipError; nothing is launched for them."""
    from drba_amd import _lib, ops
    dev = hip_backend.dev
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    for radius in (1, 3, 5):  # only the radius GMFlow's refinement stage uses
        with pytest.raises(_lib.DrbaHipError):
            ops.local_corr_flow(z(1, 128, 8, 8), z(1, 128, 8, 8), radius)
    for h, w in ((1, 8), (8, 1), (1, 1)):  # 2c / (n - 1) - 1 has no meaning for n = 1
        with pytest.raises(_lib.DrbaHipError):
            ops.flow_warp(z(1, 4, h, w), z(1, 2, h, w))
        with pytest.raises(_lib.DrbaHipError):
            ops.backwarp(z(1, 4, h, w), z(1, 2, h, w), "zeros")
        with pytest.raises(_lib.DrbaHipError):
            ops.metric_input(z(1, 3, h, w), z(1, 3, h, w), z(1, 2, h, w), z(1, 2, h, w))
    with pytest.raises(_lib.DrbaHipError):
        ops.softmax_rows_(z(2, 3, 5), 0.0)  # scale must be positive
    with pytest.raises(_lib.DrbaHipError):  # a channel slice of N = 2 is not contiguous: the gathers store through a raw pointer
        ops.softsplat(z(2, 3, 8, 8), z(2, 2, 8, 8), None, "avg", out=z(2, 6, 8, 8)[:, 1:4])
    # the IFNet stage glue: the pyramid rules that bound the staged footprints
    h, w = 32, 64
    img, f, t = z(1, 3, h, w), z(1, 16, h, w), z(1, 1, h, w)
    item = [(img, img, t, f, f)]
    ops.pair_interleaved(f)  # (the layout copy the warped entry points make of planar features on first use: not the refused launch)
    head =lambda s, n=1: z(n, 13, h // s, w // s)  # noqa: E731

    def refused(call):
        def go():
            with pytest.raises(_lib.DrbaHipError):
                call()
        _, names = _traced(go)
        assert names == [], names

    refused(lambda: ops.stage_inputs(item, None, head(4), 4.0, 2.0, z(1, 52, h // 2, w // 2), terms=[(head(4), 4.0)]))  # a term below 2 x prev_scale
    refused(lambda: ops.ifblock_input_lds(img, img, f, f, t, None, head(8), 8.0, 4.0, fold=True))                       # a fold at scale 4
    refused(lambda: ops.ifblock_input_lds(img, img, f, f, t, z(1, 4, h, w), head(4), 4.0, 1.0))                         # prev_scale != 2 x scale
    refused(lambda: ops.warp_blend_lazy([(img, img)], [(head(2), 2.0)], head(2), 2.0))                                  # a term at the last head's scale
    refused(lambda: ops.warp_blend_lazy([(img, img)], [(head(s), float(s)) for s in (32, 16, 8, 4, 2)], head(1), 1.0))  # > MAX_FLOW_TERMS terms
    assert _lib.MAX_FLOW_TERMS == 4
    # the fused window attention: a shifted window one pixel wide or high (the reference's mask table is degenerate there: the model
    # takes the drba_bmm path), a map the windows do not divide; a linear layer whose K is no multiple of the 32-feature chunk
    qkv = z(1, 140 * 2, 128)
    refused(lambda: ops.window_attention(qkv, qkv, qkv, 140, 2, 2, True, 128 ** 0.5))
    refused(lambda: ops.window_attention(qkv, qkv, qkv, 2, 140, 2, True, 128 ** 0.5))
    refused(lambda: ops.window_attention(qkv, qkv, qkv, 140, 2, 3, False, 128 ** 0.5))
    with pytest.raises(_lib.DrbaHipError):
        ops.LinearSplit(z(8, 48).cpu(), None, device=dev)  # K % 32 != 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------- the GMFlow transformer kernels
def test_window_attention_edges(hip_backend):
    """window_attn.hip with 3 and 2 terms on both sides of the key chunk, the query tiles and the 4 / 8-wave switch, odd windows with a
    shift, ww == 1, 1 to 18 windows, 1 to 6 key runs, inputs on which the -100 mask and the running rescale decide, strided views"""
    _assert_rows(op_checks.check_window_attention_edges(hip_backend.dev))


def _attn_launch(recs, c, terms):
    """(key runs per window, waves) of one traced ops.window_attention call, read from the grid and the kernel names"""
    main = [r for r in recs if "window_attention" in r["name"] and "merge" not in r["name"]]
    merges = [r for r in recs if "window_attention_merge" in r["name"]]
    assert len(main) == 1 and len(merges) <= 1, [r["name"] for r in recs]
    name = main[0]["name"]
    waves = 8 if "window_attention16_kernel<8>" in name else 4
    assert ("window_attention16_kernel<" in name) == (terms == 2), (terms, name)
    per_run = 8 * -(-c.nwin // 8) * -(-c.L // (16 * waves))
    runs, rest = divmod(main[0]["grid"][0], per_run)
    assert rest == 0 and main[0]["grid"][1:] == (1, 1) and (runs > 1) == bool(merges), (main[0]["grid"], per_run, [r["name"] for r in recs])
    return runs, waves


def test_window_attention_dispatch_forms_ran(hip_backend):
    """ATTN_RUNS (and the b = 2 shifted case that splits its keys) under the kernel trace: the run count launched is grid / (8
    ceil(nwin / 8) qtiles), the merge is in the trace exactly when it is above 1.  1..6 runs of the two-term kernel and 1, 2, 4 of the
    fp32 kernel, an uneven split of each, and both wave forms were launched -- and are what the restated rules say: a retune that
    un-covers a count fails here."""
    from drba_amd import ops
    dev = hip_backend.dev
    rows, seen = [], {2: set(), 3: set()}
    forms, uneven_seen = set(), {2: 0, 3: 0}
    for c in op_checks.ATTN_RUNS + tuple(c for c in op_checks.ATTN_GEOMETRY if c.b == 2 and op_checks.attn_runs(c, 2) > 1):
        q, k, v = [t.to(dev) for t in op_checks.attn_inputs(c)]
        for terms in (3, 2):
            out = []
            recs = _traced_recs(lambda: out.append(ops.window_attention(q, k, v, c.h, c.w, c.splits, c.shift, c.scale, terms=terms)))
            runs, waves = _attn_launch(recs, c, terms)
            print(f"  terms={terms} {c.name}: {[(r['name'], r['grid'][0]) for r in recs]} -> {runs} runs, {waves} waves")
            assert runs == op_checks.attn_runs(c, terms), (c.name, terms, runs)
            seen[terms].add(runs)
            uneven_seen[terms] += op_checks.uneven(c.L, runs)
            if terms == 2:
                forms.add(waves)
            rows.append(op_checks.attn_row("window_attention", c, terms, out[0], f"runs={runs} traced"))
    # below the switch (the geometry rows run the 4-wave form; one of them again here for the trace)
    c = next(c for c in op_checks.ATTN_GEOMETRY if c.L == 187)
    q, k, v = [t.to(dev) for t in op_checks.attn_inputs(c)]
    recs = _traced_recs(lambda: ops.window_attention(q, k, v, c.h, c.w, c.splits, c.shift, c.scale, terms=2))
    forms.add(_attn_launch(recs, c, 2)[1])
    assert seen[2] == {1, 2, 3, 4, 5, 6} and seen[3] == {1, 2, 4}, seen
    assert forms == {4, 8} and uneven_seen[2] >= 2 and uneven_seen[3] >= 2, (forms, uneven_seen)
    _assert_rows(rows)


def _attn_direct(lib, dev, c, terms, ws_mode):
    """drba_window_attention through the C ABI into out = [b, n, 128] + GUARD sentinels; ws_mode None: ws = NULL; "exact": a workspace of
    exactly drba_window_attention_ws_floats floats + GUARD sentinels -> (out values, out sentinels, ws sentinels or None, ws floats)"""
    import ctypes as C
    from drba_amd import ops
    q, k, v = [t.to(dev) for t in op_checks.attn_inputs(c)]
    n = c.b * c.h * c.w * 128
    out = torch.full((n + op_checks.GUARD,), op_checks.SENTINEL, device=dev)
    ws, size = None, 0
    if ws_mode == "exact":
        size = lib.drba_window_attention_ws_floats(c.b, c.h, c.w, c.splits)
        ws = torch.full((size + op_checks.GUARD,), op_checks.SENTINEL, device=dev)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    rc = lib.drba_window_attention(ptr(q), ptr(k), ptr(v), ptr(out), c.b, c.h, c.w, 128, c.splits, int(c.shift), float(c.scale), 128, 128, 128,
                                   ptr(ws), terms, ops._stream())
    assert rc == 0, (rc, c.name)
    torch.cuda.synchronize()
    return out[:n].view(c.b, c.h * c.w, 128), out[n:], None if ws is None else ws[size:], size


def test_window_attention_token_table_forms(hip_backend):
    """The two-term kernel walking every key of a window in one run (ws = NULL through the C ABI): 3968 keys -- kTabCap, the longest
    walk that takes the token table -- and 4032, the first that evaluates token_row per chunk with 64-bit row offsets; and four
    shifted windows of 4032 (regions from the per-chunk form).  Value rows against fp64; the trace shows one launch and no merge."""
    from drba_amd import _lib
    lib, dev = _lib.load(), hip_backend.dev
    rows = []
    sent = torch.full((op_checks.GUARD,), op_checks.SENTINEL)
    for c in op_checks.ATTN_TABLE:
        assert (c.L <= op_checks.ATTN_TAB_CAP) == (c is op_checks.ATTN_TABLE[0])  # window_attn.hip:695-698 with ksplit = 1
        got = []
        recs = _traced_recs(lambda: got.append(_attn_direct(lib, dev, c, 2, None)))
        runs, waves = _attn_launch(recs, c, 2)
        assert (runs, waves) == (1, 8), (runs, waves)
        out, tail, _, _ = got[0]
        table = "table" if c.L <= op_checks.ATTN_TAB_CAP else "token_row per chunk"
        rows.append(op_checks.attn_row("window_attention", c, 2, out, f"ws=NULL: one walk of {c.L} keys, {table}"))
        rows.append(op_checks.exact_row("window_attention", f"terms=2 {c.name}: the {op_checks.GUARD} floats behind out", tail, sent))
    _assert_rows(rows)


def test_window_attention_guards(hip_backend):
    """out and the workspace of exactly drba_window_attention_ws_floats floats each followed by 4096 sentinels, one shape per key-run
    count, both term counts: the sentinels are untouched and the values hold their fp64 row"""
    from drba_amd import _lib
    lib, dev = _lib.load(), hip_backend.dev
    rows = []
    sent = torch.full((op_checks.GUARD,), op_checks.SENTINEL)
    shapes = {}
    for c in op_checks.ATTN_RUNS + tuple(c for c in op_checks.ATTN_GEOMETRY if c.b == 2):
        shapes.setdefault((op_checks.attn_runs(c, 2), op_checks.attn_runs(c, 3), c.b), c)
    assert {k[0] for k in shapes} == {1, 2, 3, 4, 5, 6} and {k[1] for k in shapes} == {1, 2, 4}
    for c in shapes.values():
        for terms in (3, 2):
            out, tail, ws_tail, size = _attn_direct(lib, dev, c, terms, "exact")
            name = f"terms={terms} {c.name}"
            rows.append(op_checks.attn_row("window_attention", c, terms, out, f"guarded, ws={size} floats, runs={op_checks.attn_runs(c, terms)}"))
            rows.append(op_checks.exact_row("window_attention", f"{name}: the {op_checks.GUARD} floats behind out", tail, sent))
            rows.append(op_checks.exact_row("window_attention", f"{name}: the {op_checks.GUARD} floats behind the workspace", ws_tail, sent))
    _assert_rows(rows)


def test_global_expect2_edges(hip_backend):
    """global_corr.hip on both sides of the chunk and the query tile, 1 x 70 and 70 x 1 maps, w > h and h > w, 1 to 8 key runs with
    even runs of the minimum of 4 chunks and uneven splits, a late maximum, strided q and k; coordinates and a flow as values at every shape"""
    _assert_rows(op_checks.check_global_expect2_edges(hip_backend.dev))


def test_global_expect2_dispatch_and_guards(hip_backend):
    """Every map of GCORR_RUNS (and one below the first split) through the C ABI under the kernel trace, into out = [2, L] + 4096
    sentinels with a workspace of exactly drba_global_expect2_ws_floats(L) floats + 4096 sentinels: the run count launched (grid /
    qtiles; the merge in the trace exactly above 1) is what the restated rule says, 1..8 were all launched, the sentinels are
    untouched and the values hold their rows."""
    import ctypes as C
    from drba_amd import _lib, ops
    lib, dev = _lib.load(), hip_backend.dev
    rows, seen, even_min = [], set(), {}
    sent = torch.full((op_checks.GUARD,), op_checks.SENTINEL)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    maps = [(m, op_checks.GCORR_SEEDS[m]) for m in op_checks.GCORR_MAPS[:1] + op_checks.GCORR_RUNS]
    for (h, w), seed in maps:
        L = h * w
        t0, t1, flow = [t.to(dev) for t in op_checks.gcorr_inputs(h, w, seed)]
        size = lib.drba_global_expect2_ws_floats(L)
        got = {}
        for what, vals in (("coords", None), ("values", flow)):
            out = torch.full((2 * L + op_checks.GUARD,), op_checks.SENTINEL, device=dev)
            ws = torch.full((size + op_checks.GUARD,), op_checks.SENTINEL, device=dev)
            recs = _traced_recs(lambda: got.__setitem__("rc", lib.drba_global_expect2(ptr(t0), ptr(t1), ptr(vals), ptr(out), ptr(ws), L, 128, w,
                                                                                 float(op_checks.S128), 128, 128, ops._stream())))
            assert got["rc"] == 0
            main = [r for r in recs if "global_expect2_kernel" in r["name"]]
            merges = [r for r in recs if "global_expect2_merge" in r["name"]]
            assert len(main) == 1 and len(merges) <= 1, (L, recs)
            runs, rest = divmod(main[0]["grid"][0], -(-L // op_checks.ATTN_ROWS))
            assert rest == 0 and (runs > 1) == (len(merges) == 1) and runs == op_checks.gcorr_ksplit(L), (L, recs)
            even_min[runs] = even_min.get(runs, False) or -(-L // op_checks.ATTN_KEYS) == 4 * runs
            seen.add(runs)
            got[what] = out[:2 * L].view(2, L)
            name = f"{what} {h}x{w} (L={L}) runs={runs}"
            rows.append(op_checks.exact_row("global_expect2", f"{name}: the {op_checks.GUARD} floats behind out", out[2 * L:], sent))
            rows.append(op_checks.exact_row("global_expect2", f"{name}: the {op_checks.GUARD} floats behind the {size}-float workspace", ws[size:], sent))
        rows.extend(op_checks.gcorr_rows("global_expect2", f"{h}x{w} (L={L}) guarded, traced", h, w, got["coords"], got["values"],
                                         op_checks.gcorr_refs(h, w, seed)))
    assert seen == {1, 2, 3, 4, 5, 6, 7, 8}, seen
    assert all(even_min[k] for k in range(2, 9)), even_min  # each count also as even runs of the minimum of 4 chunks
    _assert_rows(rows)


def test_strided_views_reach_the_kernels_in_place(hip_backend, monkeypatch):
    """The bit-equality rows on strided views say something only while ops.window_attention, ops.global_expect2 and LinearSplit.cat
    hand the views themselves to the library: every pointer the wrappers pass goes through ops._p, so each view's address must be
    among them -- a wrapper that started to copy such a view would pass the address of the copy and fail here."""
    from drba_amd import ops
    dev = hip_backend.dev
    passed, real = set(), ops._p
    monkeypatch.setattr(ops, "_p", lambda t: (passed.add(None if t is None else t.data_ptr()), real(t))[1])
    for strided in (op_checks.attn_strided_rows, op_checks.gcorr_strided_rows, op_checks.lin_cat_rows):
        views = []
        passed.clear()
        rows = strided(dev, ops, views)
        torch.cuda.synchronize()
        assert len(views) >= 2 and not any(v.is_contiguous() for v in views)
        missing = [(tuple(v.shape), v.stride()) for v in views if v.data_ptr() not in passed]
        assert not missing, f"{strided.__name__}: views copied before the call: {missing}"
        _assert_rows(rows)


def test_linear_split_edges(hip_backend):
    """linear_split.hip with 3 and 2 terms at the token and feature tile edges, one K chunk, cat splits at the first and last chunk
    on strided views, the 128-token form and the shape below it, GELU over [-12, 12], LayerNorm rows of variance 0 and of mean 100"""
    _assert_rows(op_checks.check_linear_split_edges(hip_backend.dev))


def test_linear_split_tile_forms_ran(hip_backend):
    """K = 32, N = 4096, two terms: M = 6100 is 48 x 32 = 1536 workgroups of 128 x 128 (wide_min, linear_split.hip:309-310) and runs
    LinCfg<2, 8, 2> with a ragged last 128-token tile, M = 6016 (1504) runs LinCfg<1, 8, 2> -- read from the traced kernel names, for
    the plain and the GELU epilogue.  (The LayerNorm epilogue has one feature tile: its wide form needs M >= 196 481.)"""
    import re
    from drba_amd import ops
    dev = hip_backend.dev
    k, n = op_checks.LIN_WIDE_KN
    x = op_checks.cases.rnd((op_checks.LIN_WIDE[0][0], k), 5350, 2.0).to(dev)
    w = op_checks.cases.rnd((n, k), 5351, 1.0 / k ** 0.5)
    for gelu in (False, True):
        layer = ops.LinearSplit(w, None, gelu=gelu, device=dev, terms=2)
        layer.packed
        for m, wide in op_checks.LIN_WIDE:
            assert (-(-m // 128) * -(-n // 128) >= op_checks.LIN_WIDE_MIN) == wide
            recs = _traced_recs(lambda: layer(x[:m]))
            names = [r["name"] for r in recs if "linear_split_kernel" in r["name"]]
            print(f"  M={m} gelu={int(gelu)}: {names} grid {[r['grid'] for r in recs]}")
            assert len(names) == 1 and re.search(rf"LinCfg<{2 if wide else 1}, ?8, ?2>, ?{int(gelu)}>", names[0]), names
            assert recs[0]["grid"][0] == -(-m // (128 if wide else 64)) * (n // 128)
    torch.cuda.synchronize()


def test_linear_split_guards(hip_backend):
    """drba_linear_split, _cat and _layernorm through the C ABI into out = [M, N] + 4096 sentinels at M = 65, N = 129 and M = 129,
    N = 128, both term counts: sentinels untouched, values at the project's bar"""
    import ctypes as C
    from drba_amd import _lib, ops
    lib, dev = _lib.load(), hip_backend.dev
    rows = []
    sent = torch.full((op_checks.GUARD,), op_checks.SENTINEL)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    rnd = op_checks.cases.rnd
    for i, (m, n) in enumerate(((65, 129), (129, 128))):
        k1, k2 = 32, 64
        k = k1 + k2
        x, w, b = rnd((m, k), 5500 + 5 * i, 2.0), rnd((n, k), 5501 + 5 * i, 1.0 / k ** 0.5), rnd((n,), 5502 + 5 * i, 0.5)
        lw, lb, res = rnd((128,), 5503 + 5 * i, 0.3) + 1.0, rnd((128,), 5504 + 5 * i, 0.1), rnd((m, 128), 5505 + 5 * i, 1.0)
        xd, x1, x2 = x.to(dev), x[:, :k1].contiguous().to(dev), x[:, k1:].contiguous().to(dev)
        lwd, lbd, resd = lw.to(dev), lb.to(dev), res.to(dev)
        for terms in (3, 2):
            layer = ops.LinearSplit(w, b, device=dev, terms=terms)
            calls = {
                "linear": lambda o: lib.drba_linear_split(ptr(xd), ptr(layer.packed), ptr(layer.bias), ptr(o), m, k, n, k, 0, terms, ops._stream()),
                "linear + GELU": lambda o: lib.drba_linear_split(ptr(xd), ptr(layer.packed), ptr(layer.bias), ptr(o), m, k, n, k, 1, terms, ops._stream()),
                "cat": lambda o: lib.drba_linear_split_cat(ptr(x1), ptr(x2), ptr(layer.packed), ptr(layer.bias), ptr(o), m, k1, k2, n, k1, k2, 0, terms,
                                                            ops._stream())}
            if n == 128:
                calls["LayerNorm"] = lambda o: lib.drba_linear_split_layernorm(ptr(xd), ptr(layer.packed), ptr(layer.bias), ptr(lwd), ptr(lbd), ptr(resd),
                                                                               ptr(o), m, k, k, 1e-5, terms, ops._stream())
            for what, call in calls.items():
                out = torch.full((m * n + op_checks.GUARD,), op_checks.SENTINEL, device=dev)
                assert call(out) == 0
                torch.cuda.synchronize()
                if what == "LayerNorm":
                    r64, r32, bar = op_checks._ln_ref(*op_checks._dbl(x, w, b, lw, lb, res)), op_checks._ln_ref(x, w, b, lw, lb, res), 1e-5
                else:
                    r64, r32, bar = op_checks._lin_ref(*op_checks._dbl(x, w, b), what.endswith("GELU")), op_checks._lin_ref(x, w, b, what.endswith("GELU")), 5e-6
                name = f"terms={terms} {what} [{m}x{k}] -> {n} guarded"
                rows.append(op_checks.lin_row("linear_split", name, out[:m * n].view(m, n), r64, r32, bar))
                rows.append(op_checks.exact_row("linear_split", f"{name}: the {op_checks.GUARD} floats behind out", out[m * n:], sent))
    _assert_rows(rows)


# ----------------------------------------------------------------------------------------- the fused IFNet encoder
HEAD_GUARDED = ((2, 4), (6, 12), (130, 4), (16, 516))  # single frames of op_checks.HEAD_CASES that also run into guarded outputs
HEAD_FORMS = ((False, "fp32", ""), (True, "two-term", "16"))  # (HEAD_TWO_TERM, row label, suffix of the entry point and of the holder's pack)


def _drain_status(ops, dev):
    """the device's overflow word asked for, every kernel finished, and whatever earlier tests left taken out of it"""
    ops.status_init(dev)
    torch.cuda.synchronize()
    ops.overflow_groups(dev)


def test_head_fused(hip_backend):
    """head_fused.hip and head_fused16.hip on the nine shapes of op_checks.HEAD_CASES (the smallest frame, one tile, one position past it,
    exactly the rings in the second tile, an interior tile with W % 8 == 4 and == 0, nine tiles in a row and in a column), on zero,
    signed 1e3 / 1e-3 and (fp32) NaN-pixel frames: planar against fp64 under the one rule, both layouts and the planar=False call bit for
    bit.  Nothing of it is reported as an overflow: every input is inside the two-term form's documented range."""
    from drba_amd import ops
    dev = hip_backend.dev
    _drain_status(ops, dev)
    rows = op_checks.check_head_fused(dev)
    torch.cuda.synchronize()
    reported = ops.overflow_groups(dev)
    for form in ("fp32", "two-term"):
        worst = max((r for r in rows if r.floor is not None and f" {form} " in r[0]), key=lambda r: r[1] / r[2])
        print(f"  largest err / tol, {form}: {worst[1] / worst[2]:.3f} ({worst[0]})")
    _assert_rows(rows)
    assert reported == [], reported


def test_head_fused_forms_ran(hip_backend):
    """Under the kernel trace: with HEAD_TWO_TERM False every call is one launch of head_fused, with True one of head_fused16, planar
    or pair-only, on a grid of (tiles_x * tiles_y, 1) -- the tile counts the case table's edge conditions are computed from."""
    from drba_amd import ops
    dev = hip_backend.dev
    seen = set()
    try:
        for two, form, sfx in HEAD_FORMS:
            ops.HEAD_TWO_TERM = two
            layers, holder = op_checks.head_layers(ops, dev, "synth")
            for h, w, _ in op_checks.HEAD_CASES:
                x = op_checks.head_refs(h, w, "rand")["x"].to(dev)
                nx, ny = op_checks.head_tiles(h, w)
                for planar in (True, False):
                    recs = _traced_recs(lambda: ops.head_fused(x, layers, holder, planar=planar))
                    print(f"  {form} {h}x{w} planar={int(planar)}: {[(r['name'], tuple(r['grid'])) for r in recs]}")
                    assert len(recs) == 1 and "head_fused" in recs[0]["name"], recs
                    assert ("head_fused16" in recs[0]["name"]) == two, (two, recs[0]["name"])
                    assert tuple(recs[0]["grid"][:2]) == (nx * ny, 1), (h, w, recs[0]["grid"])
                    seen.add(recs[0]["name"])
    finally:
        ops.HEAD_FUSED, ops.HEAD_TWO_TERM = True, None
    assert len(seen) == 2, seen


def test_head_fused_batch_and_guards(hip_backend):
    """drba_head_fused / drba_head_fused16 through the C ABI with N = 3 different 18 x 68 frames (blockIdx.y offsets of 3 P and 16 P),
    f_out and f_pair_out each in the middle of a NaN-prefilled allocation between sentinels: every item against fp64 and bit for bit
    equal to the N = 1 launch of its frame, no NaN left (every element written), the sentinels untouched; then f_out = NULL, which
    leaves the same f_pair_out; then the four most cut single frames (HEAD_GUARDED) between the same sentinels."""
    import ctypes as C
    from drba_amd import _lib, ops
    lib, dev = _lib.load(), hip_backend.dev
    n, h, w = op_checks.HEAD_BATCH
    r = op_checks.head_refs(h, w, "rand", n)
    x = r["x"].to(dev)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    op, rows = "head_fused", []
    nx, ny = op_checks.head_tiles(h, w)
    try:
        for two, form, sfx in HEAD_FORMS:
            ops.HEAD_TWO_TERM = two
            layers, holder = op_checks.head_layers(ops, dev, "synth")
            singles = [ops.head_fused(x[k:k + 1].clone(), layers, holder) for k in range(n)]  # the N = 1 launches (the first packs the weights)
            pk, launch = getattr(holder, "_fused_pack" + sfx), getattr(lib, "drba_head_fused" + sfx)
            name = f"{form} N={n} {h}x{w}"
            bf, f = op_checks.conv_guarded((n, 16, h, w), dev)
            bp, fp = op_checks.conv_guarded((n, 8, h, w, 2), dev)
            rc = []
            recs = _traced_recs(lambda: rc.append(launch(ptr(x), ptr(pk), ptr(f), ptr(fp), n, h, w, ops._stream())))
            print(f"  {name}: {[(q['name'], tuple(q['grid'])) for q in recs]}")
            assert rc == [0] and len(recs) == 1 and tuple(recs[0]["grid"][:2]) == (nx * ny, n), (rc, recs)
            for k in range(n):
                rows.append(op_checks.value_row(op, f"{name} item {k}: planar vs fp64", f[k:k + 1], r["ref64"][k:k + 1], r["ref32"][k:k + 1]))
                rows.append(op_checks.exact_row(op, f"{name} item {k}: planar == the N=1 launch of frame {k}", f[k:k + 1], singles[k]))
                rows.append(op_checks.exact_row(op, f"{name} item {k}: pair layout == the N=1 launch of frame {k}", fp[k], singles[k]._drba_pair))
            left = int(f.isnan().sum()) + int(fp.isnan().sum())
            rows.append(op_checks.Row(op, f"{name}: NaN left of the prefill in f_out / f_pair_out", float(left), 0.0, "every element written"))
            rows.append(op_checks.guard_row(op, f"{name} f_out", bf))
            rows.append(op_checks.guard_row(op, f"{name} f_pair_out", bp))
            bp2, fp2 = op_checks.conv_guarded((n, 8, h, w, 2), dev)
            assert launch(ptr(x), ptr(pk), ptr(None), ptr(fp2), n, h, w, ops._stream()) == 0
            torch.cuda.synchronize()
            rows.append(op_checks.exact_row(op, f"{name} f_out=NULL: f_pair_out == the launch that also writes planes", fp2, fp))
            rows.append(op_checks.guard_row(op, f"{name} f_out=NULL f_pair_out", bp2))
            # the frames whose last tile is cut the most, one each, between the same sentinels: the smallest, one tile with a half
            # tile's tail, nine tiles in a column of a 4-pixel row, nine in a row with the tail in the narrow last strip
            for gh, gw in HEAD_GUARDED:
                g = op_checks.head_refs(gh, gw, "rand")
                xg = g["x"].to(dev)
                bf, f = op_checks.conv_guarded((1, 16, gh, gw), dev)
                bp, fp = op_checks.conv_guarded((8, gh, gw, 2), dev)
                assert launch(ptr(xg), ptr(pk), ptr(f), ptr(fp), 1, gh, gw, ops._stream()) == 0
                torch.cuda.synchronize()
                rows.append(op_checks.head_value_row(op, f"{form} guarded {gh}x{gw}: planar vs fp64", f, g, two))
                rows.append(op_checks.exact_row(op, f"{form} guarded {gh}x{gw}: pair layout == the pair layout of the planar result", fp, op_checks.pair_layout(f)))
                rows.append(op_checks.guard_row(op, f"{form} guarded {gh}x{gw} f_out", bf))
                rows.append(op_checks.guard_row(op, f"{form} guarded {gh}x{gw} f_pair_out", bp))
    finally:
        ops.HEAD_FUSED, ops.HEAD_TWO_TERM = True, None
    _assert_rows(rows)


def test_head_fused16_nan_pixel(hip_backend):
    """The NaN pixel at the seam of four tiles in the two-term form: NaN in exactly the cone the reference has (rows 9..22, columns
    57..70, all 16 channels), fp64 values elsewhere, both layouts alike -- and the kernel reports the NaN it stored: the status word
    names head_fused16 and nothing else.  Reading it takes it back, so later tests see the word clean."""
    from drba_amd import ops
    dev = hip_backend.dev
    h, w = op_checks.HEAD_NAN[:2]
    r = op_checks.head_refs(h, w, "NaN pixel")
    _drain_status(ops, dev)
    try:
        ops.HEAD_TWO_TERM = True
        layers, holder = op_checks.head_layers(ops, dev, "synth")
        x = r["x"].to(dev)
        (f, f2), names = _traced(lambda: (ops.head_fused(x, layers, holder), ops.head_fused(x, layers, holder, planar=False)))
        groups = ops.overflow_groups(dev)  # (_traced synchronises: both launches are done)
    finally:
        ops.HEAD_FUSED, ops.HEAD_TWO_TERM = True, None
    assert len(names) == 2 and all("head_fused16" in k for k in names), names
    (ra, rb), (ca, cb) = op_checks.HEAD_NAN_CONE
    want = torch.zeros(1, 16, h, w, dtype=torch.bool)
    want[:, :, ra:rb + 1, ca:cb + 1] = True
    name = f"two-term NaN pixel {h}x{w}"
    rows = [op_checks.head_value_row("head_fused", f"{name}: planar vs fp64", f, r, True),
            op_checks.exact_row("head_fused", f"{name}: NaN exactly in rows {ra}..{rb} x columns {ca}..{cb}", f.isnan(), want),
            op_checks.exact_row("head_fused", f"{name}: pair copy == the pair layout of the planar result", f._drba_pair, op_checks.pair_layout(f)),
            op_checks.exact_row("head_fused", f"{name}: planar=False == the pair copy of the planar call", f2, f._drba_pair)]
    print(f"  reported: {groups}")
    _assert_rows(rows)
    assert groups == ["head_fused16"], groups
    assert ops.overflow_groups(dev) == []


def test_head_fused_refusals(hip_backend):
    """The return codes of both entry points on tiny real buffers: DRBA_EUNSUPPORTED (-2) for odd H, W % 4 != 0 and N > 65535,
    DRBA_EINVAL (-1) for N = 0, H = 0 and an output that is not 16-byte aligned -- nothing is launched for any of them -- and 0 for the
    smallest frame, N = 1, H = 2, W = 4, which launches one workgroup."""
    import ctypes as C
    from drba_amd import _lib, ops
    lib, dev = _lib.load(), hip_backend.dev
    x = op_checks.head_refs(2, 4, "rand")["x"].to(dev)
    f, fp = torch.zeros(16 * 2 * 4 + 4, device=dev), torch.zeros(16 * 2 * 4 + 4, device=dev)
    at = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    try:
        for two, form, sfx in HEAD_FORMS:
            ops.HEAD_TWO_TERM = two
            layers, holder = op_checks.head_layers(ops, dev, "synth")
            want = ops.head_fused(x, layers, holder)  # (packs the weights)
            pk, launch = getattr(holder, "_fused_pack" + sfx), getattr(lib, "drba_head_fused" + sfx)
            call = lambda n, h, w, fo=0, po=0: launch(at(x), at(pk), at(f, fo), at(fp, po), n, h, w, ops._stream())  # noqa: E731
            table = (("H = 7", lambda: call(1, 7, 4), -2), ("W = 10", lambda: call(1, 2, 10), -2), ("N = 65536", lambda: call(65536, 2, 4), -2),
                     ("N = 0", lambda: call(0, 2, 4), -1), ("H = 0", lambda: call(1, 0, 4), -1),
                     ("f_pair_out + 4 bytes", lambda: call(1, 2, 4, po=4), -1), ("f_out + 4 bytes", lambda: call(1, 2, 4, fo=4), -1),
                     ("N = 1, H = 2, W = 4", lambda: call(1, 2, 4), 0))
            for what, go, code in table:
                rc, names = _traced(go)
                print(f"  {form} {what}: {rc}, launched {names}")
                assert rc == code, (form, what, rc, code)
                assert len(names) == (1 if code == 0 else 0), (form, what, names)
            torch.cuda.synchronize()
            assert op_checks._mismatches(f[:16 * 2 * 4].view(1, 16, 2, 4), want) == 0 and float(f[16 * 2 * 4:].abs().max()) == 0.0
    finally:
        ops.HEAD_FUSED, ops.HEAD_TWO_TERM = True, None


def test_head_fused_fallback_runs_the_layers(hip_backend):
    """What ops.head_fused does not take -- a batch of two (16 x 24), odd H (17 x 36), W % 4 == 2 (18 x 70) -- goes through Head's
    layer chain: Head(x) holds the fp64 layers under the same rule, and the trace shows layer kernels and no head_fused launch."""
    from drba_amd import ops
    from drba_amd.models.rife_426_heavy.IFNet_HDv3 import Head
    from drba_amd.utils import synth
    dev = hip_backend.dev
    head = Head(synth.ifnet_state_dict(seed=0), "encode.", dev)
    wts = op_checks.head_weights("synth")
    rows = []
    assert ops.HEAD_FUSED is True and ops.HEAD_TWO_TERM is None
    for n, h, w in op_checks.HEAD_REFUSED:
        x = op_checks.head_frame(h, w, "rand", n)
        got, names = _traced(lambda: head(x.to(dev)))
        print(f"  [{n}, 3, {h}, {w}]: {sorted(set(names))}")
        assert names and not any("head_fused" in k for k in names), names
        rows.append(op_checks.value_row("head_fused", f"Head([{n}, 3, {h}, {w}]) through the layer chain vs fp64", got, op_checks.head_ref(x, wts),
                                        op_checks.head_ref(x, wts, torch.float32)))
    _assert_rows(rows)


# ----------------------------------------------------------------------------------------- the fused RIFE splats
@pytest.mark.parametrize("group", op_checks.RIFE_GROUPS)
def test_rife_splats(hip_backend, group):
    """splat_long_prepass / splat_tiled and their _det forms -- all of flow_reverse, drm_rife_linear(_many) and drm_rife_nonlinear(_many)
    -- against fp64 under the two-branch rule, at the 2e-4 / 2e-5 bars these entry points already hold, one case group per test:
    the window edges of every halo variant, the reach rounding, neighbour reach, long sources and the flags, the record capacity,
    small maps, non-finite and far flows, items.  Each group in the default and in the deterministic mode."""
    rows = op_checks.check_rife_splats(hip_backend.dev, groups=(group,))
    assert {r.group for r in rows} == {group} and any(" det" in r[0] for r in rows)
    _assert_rows(rows)


def _fused_launches(recs):
    fused = [r for r in recs if r["name"].startswith(("splat_long_prepass", "splat_tiled"))]
    other = sorted({r["name"] for r in recs} - {r["name"] for r in fused})
    return fused, other


def test_rife_splats_launch_the_fused_kernels(hip_backend):
    """From the launch trace: a default-mode group launches splat_long_prepass and splat_tiled in pairs and nothing else -- no
    generic splat, no composition --, a deterministic one the _det pair."""
    dev = hip_backend.dev
    for det, pre, tile in ((False, "splat_long_prepass<", "splat_tiled<"), (True, "splat_long_prepass_det<", "splat_tiled_det<")):
        rows = []
        recs = _traced_recs(lambda: rows.extend(op_checks.check_rife_splats(dev, groups=("neighbour", "nonfinite", "small", "long"), modes=(det,))))
        fused, other = _fused_launches(recs)
        print(f"  det={det}: {sorted({r['name'] for r in fused})} other: {other}")
        assert not other, other
        assert len(fused) >= 2 * 9 and len(fused) % 2 == 0
        for a, b in zip(fused[0::2], fused[1::2]):
            assert a["name"].startswith(pre) and b["name"].startswith(tile) and a["grid"] == b["grid"], (a, b)
        _assert_rows(rows)


def test_rife_splats_without_the_reach_map(hip_backend):
    """flow_reverse at N * tiles == REACH_WORDS and at one tile row more per item, where the kernels skip the reach map and every tile
    scans the 16-pixel halo (op_checks.check_rife_splats_nomap: 12.6 M pixels, 0.7 GB on the device; fp64 on three items).  The
    trace shows that the second geometry did launch more than REACH_WORDS workgroups, in both modes, and the first exactly that many."""
    from tests import det_common
    rows = []
    recs = _traced_recs(lambda: rows.extend(op_checks.check_rife_splats_nomap(hip_backend.dev)))
    fused, other = _fused_launches(recs)
    assert not [n for n in other if "splat" in n], other
    groups = {}
    for r in fused:
        groups.setdefault(r["name"], set()).add(r["grid"][0] * r["grid"][1] * r["grid"][2])
    print("  " + "\n  ".join(f"{k}: workgroups {sorted(v)}" for k, v in sorted(groups.items())))
    n, h = op_checks.nomap_geometry(det_common.REACH_WORDS, False)
    for name in ("splat_long_prepass<0>", "splat_tiled<0>", "splat_long_prepass_det<0>", "splat_tiled_det<0>"):
        assert det_common.REACH_WORDS in groups[name] and max(groups[name]) == n * ((h + 15) // 16) > det_common.REACH_WORDS, (name, groups[name])
    _assert_rows(rows)
