"""GPU (-m gpu): every pointwise / gather / reduction kernel of the GMFlow and GMFSS glue, the generic forward splat
(count, scan, fill, gathers), resize_bilinear_scale, flow_distance and the IFNet stage glue (stage-input gathers, the gathers
fused with conv0[0], flow update, final warp + blend: [H,W,4] frames, pair-only features, the flow as terms, the blend at the
frame's own resolution) on their own against a float64 reference (tests/op_checks.py), at the sizes where kernels go wrong:
image borders, partial tiles and blocks, every dispatch branch, batch > 1, grid-stride loops and scan rounds that go round
twice.  One operator family per test, so that a failure names it.  The 3x3 convolution's epilogue forms (op_checks.CONV_FORMS: what
the GMFlow / GMFSS layers construct) run with every configuration id pinned, one test per kernel family and form group.

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
    torch.cuda.synchronize()
