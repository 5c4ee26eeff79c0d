"""GPU (-m gpu): the batched stage kernels take their (tile, item) from csrc/common.hpp tile_item_order.  What a kernel writes
for a tile does not depend on which workgroup computes it, so ONE launch of n items must be bit-identical (torch.equal) to n
launches of one item each on the same inputs -- a wrong item, a tile computed twice or never, or a tile of another item's
geometry shows as a difference.  (Against fp64 the same kernels are covered by tests/test_gpu_parity.py.)

Shapes by their tile counts (the scale-2 fused kernel: 7 x 16 conv outputs of a quarter-resolution map per tile):
  64 x 128: 6 scale-2 tiles, fewer than XCDs; 96 x 160: 12, and with 3 items the 36 workgroups give XCD ranges that cut
  through a tile's items; 64 x 608: 10 tile columns (a full strip of 8 and a narrower one), 30 tiles.  None is a multiple of 8."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 128), (96, 160), (64, 608)]
COUNTS = [2, 3, 8]
B = 8


class Inputs:
    """8 items of one frame size: frames (with their [H,W,4] copies), encoder features, timestep maps, head outputs of
    the pyramid [B,13,H/s,W/s] for s = 32 .. 1 (flow deltas of a few pixels), two first convolutions (16 and 32 outputs)."""

    def __init__(self, dev, H, W):
        from drba_amd import ops
        g = torch.Generator().manual_seed(1000 * H + W)
        self.H, self.W = H, W
        img0, img1 = torch.rand(B, 3, H, W, generator=g).to(dev), torch.rand(B, 3, H, W, generator=g).to(dev)
        f0, f1 = torch.randn(B, 16, H, W, generator=g).to(dev), torch.randn(B, 16, H, W, generator=g).to(dev)
        tm = torch.rand(B, 1, H, W, generator=g).to(dev)
        # per-item tensors made ONCE: the layout copies (pair-interleaved features, [H,W,4] frames) are kept on the tensor objects
        self.items = [(img0[k:k + 1], img1[k:k + 1], tm[k:k + 1], f0[k:k + 1], f1[k:k + 1]) for k in range(B)]
        for it in self.items:
            ops.rgbx(it[0]), ops.rgbx(it[1])
        self.heads = {}
        for s in (32, 16, 8, 4, 2, 1):
            t = torch.randn(B, 13, H // s, W // s, generator=g)
            t[:, :4] *= 2.0 / s  # the update is up(t[:, :4]) * s: a few pixels per stage
            self.heads[s] = t.to(dev)
        self.conv = {c: ops.Conv3x3(torch.randn(c, 52, 3, 3, generator=g) / (52 * 9) ** 0.5, torch.randn(c, generator=g) * 0.1, 2, True,
                                    None, device=dev) for c in (16, 32)}
        self._single = {}

    def terms(self, scales, a, b):
        return [(self.heads[s][a:b], float(s)) for s in scales]

    def run(self, kernel, a, b):
        """items a..b-1 in one launch -> [b - a, ...]"""
        from drba_amd import ops
        items, H, W = self.items[a:b], self.H, self.W
        if kernel in ("stage_conv16_s2", "stage_conv16", "stage_conv0"):
            ops.STAGE_CONV_TWO_TERM = kernel != "stage_conv0"
            try:
                if kernel == "stage_conv16_s2":
                    assert ops.stage_conv0_ok(self.conv[32], H, W, 2.0, 4.0, items=items)
                    y, _ = ops.stage_conv0(items, None, self.heads[4][a:b], 4.0, self.conv[32], terms=self.terms((16, 8), a, b), scale=2)
                else:
                    assert ops.stage_conv0_ok(self.conv[16], H, W, 1.0, 2.0, items=items)
                    y, _ = ops.stage_conv0(items, None, self.heads[2][a:b], 2.0, self.conv[16], terms=self.terms((16, 8, 4), a, b))
            finally:
                ops.STAGE_CONV_TWO_TERM = None
            return y
        if kernel in ("ifblock_input_lazy_s2", "ifblock_input_lazy_s8"):
            s = 2 if kernel.endswith("s2") else 8
            xin = torch.empty(b - a, 52, H // s, W // s, device=items[0][0].device)
            ops.stage_inputs(items, None, self.heads[2 * s][a:b], 2.0 * s, float(s), xin, terms=self.terms((16, 8) if s == 2 else (32,), a, b))
            return xin
        if kernel == "warp_blend_lazy":  # the last head output at half resolution: the staged form
            return torch.cat(ops.warp_blend_lazy([(it[0], it[1]) for it in items], self.terms((16, 8, 4), a, b), self.heads[2][a:b], 2.0))
        assert kernel == "warp_blend_lazy_s1"  # ... at the frame's own resolution: what the pipeline's last stage runs
        return torch.cat(ops.warp_blend_lazy([(it[0], it[1]) for it in items], self.terms((8, 4, 2), a, b), self.heads[1][a:b], 1.0))

    def single(self, kernel):
        """every item in a launch of its own, once per kernel: the reference of all item counts"""
        if kernel not in self._single:
            self._single[kernel] = torch.cat([self.run(kernel, k, k + 1) for k in range(B)]).clone()
        return self._single[kernel]


_inputs = {}


@pytest.fixture
def inputs(hip_backend, request):
    H, W = request.param
    if (H, W) not in _inputs:
        _inputs[(H, W)] = Inputs(hip_backend.dev, H, W)
    return _inputs[(H, W)]


KERNELS = ["stage_conv16_s2", "stage_conv16", "stage_conv0", "ifblock_input_lazy_s2", "ifblock_input_lazy_s8", "warp_blend_lazy",
           "warp_blend_lazy_s1"]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("inputs", SHAPES, indirect=True, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_launch_of_n_items_equals_n_launches_of_one(inputs, kernel, n):
    ref = inputs.single(kernel)
    got = inputs.run(kernel, 0, n)
    torch.cuda.synchronize()
    assert got.shape == ref[:n].shape
    assert torch.isfinite(got).all()
    assert float(ref[:n].abs().max()) > 0
    for k in range(n):
        assert torch.equal(got[k], ref[k]), f"{kernel} at {inputs.H}x{inputs.W}: item {k} of a launch of {n} differs from its own launch " \
                                            f"(max |d| {float((got[k] - ref[k]).abs().max()):.3e})"
