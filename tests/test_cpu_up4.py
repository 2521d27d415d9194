"""Host side of the four-tap form of a convolution behind a nearest-2x upsample (mvd_gemm_desc.tap_mode = MVD_TAPS_UP4): after the
upsample the 3x3 window of output pixel (2i + a, 2j + c) covers a 2x2 block of low-resolution pixels, so each output parity is a 2x2
convolution of the LOW-resolution image with the 3x3 taps that land on one pixel summed.  Checked in float64 on the CPU: the composed
weights of hip.up4_schedule, walked in its k order, against conv2d(nearest2x(x))."""
import pytest
import torch
import torch.nn.functional as F

from mvdfusion_amd import hip


def g(seed):
    return torch.Generator().manual_seed(seed)


def _walk_schedule(x, wq, order, Cout):
    """out (B, 2H, 2W, Cout): for every listed (parity, 32-channel block, tap) k-tile, the block's channels of the low-resolution image
    shifted by the tap (rows i - 1 + a + dy, columns j - 1 + c + dx; outside = zero padding) times that composed weight block."""
    B, Cin, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(B, 2 * H, 2 * W, Cout, dtype=torch.float64)
    for par, cb, tap in order:
        a, c, dy, dx = par >> 1, par & 1, tap >> 1, tap & 1
        blk = xp[:, cb * 32:(cb + 1) * 32, a + dy:a + dy + H, c + dx:c + dx + W].permute(0, 2, 3, 1)
        out[:, a::2, c::2] += blk @ wq[par][:, cb * 32:(cb + 1) * 32, dy, dx].t()
    return out


@pytest.mark.parametrize("B,H,W", [(2, 3, 5), (1, 1, 1), (3, 2, 6), (1, 4, 4)])
@pytest.mark.parametrize("Cin", [32, 96])
@pytest.mark.parametrize("Cout", [16, 40])
def test_four_composed_taps_equal_conv_of_the_upsampled_image(B, H, W, Cin, Cout):
    x = torch.randn(B, Cin, H, W, generator=g(1), dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g(2), dtype=torch.float64)
    b = torch.randn(Cout, generator=g(3), dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    wq, order = hip.up4_schedule(w)
    assert wq.dtype == torch.float64 and tuple(wq.shape) == (4, Cout, Cin, 2, 2)
    got = (_walk_schedule(x, wq, order, Cout) + b).permute(0, 3, 1, 2)
    assert float((got - ref).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("Cin", [32, 96, 1280])
def test_schedule_lists_every_weight_block_once_in_k_order(Cin):
    wq, order = hip.up4_schedule(torch.rand(8, Cin, 3, 3, generator=g(4)) + 0.5)
    assert len(order) == len(set(order)) == 16 * Cin // 32
    assert order == [(par, cb, tap) for par in range(4) for cb in range(Cin // 32) for tap in range(4)]
    # every block is a real (non-zero) weight block: positive taps sum to positive weights
    assert all(bool((wq[par][:, cb * 32:(cb + 1) * 32, tap >> 1, tap & 1] > 0).all()) for par, cb, tap in order)


def test_composed_weights_are_the_float64_sums_rounded_once():
    w = torch.randn(5, 32, 3, 3, generator=g(5))          # fp32, as the module holds it
    wq, _ = hip.up4_schedule(w)
    assert wq.dtype == torch.float32
    d = w.double()
    # parity (a, c) = (0, 1): rows {w[0]}, {w[1] + w[2]}; columns {w[0] + w[1]}, {w[2]}
    assert torch.equal(wq[1][:, :, 0, 0], (d[:, :, 0, 0] + d[:, :, 0, 1]).float())
    assert torch.equal(wq[1][:, :, 1, 0], (d[:, :, 1, 0] + d[:, :, 1, 1] + d[:, :, 2, 0] + d[:, :, 2, 1]).float())
    assert torch.equal(wq[1][:, :, 1, 1], (d[:, :, 1, 2] + d[:, :, 2, 2]).float())
    assert torch.equal(wq[2][:, :, 1, 1], (d[:, :, 2, 1] + d[:, :, 2, 2]).float())          # (1, 0): rows {w[0] + w[1]}, {w[2]}; columns {w[0]}, {w[1] + w[2]}


def test_rule_and_descriptor():
    assert hip.TAPS_UP4 == 1 and (hip.TAPS_FULL, hip.TAPS_CENTRE_TAIL) == (0, 2)
    names = [f[0] for f in hip.GemmDesc._fields_]
    assert names[-4:] == ["tap_mode", "A2", "lda2", "Cin2"] and len(names) == 76          # the four-tap form adds no descriptor field
    # training forwards and images whose low-resolution size is no multiple of 16 stay nine-tap
    assert not hip.use_up4(1 << 20, 16, 16, training=True) and not hip.use_up4(1 << 20, 3, 5)
    assert hip.use_up4(hip.UP4_MIN_ROWS, 4, 4) == (hip.UP4_MIN_ROWS > 0)
