"""Host side of the conv tap schedule (mvd_gemm_desc.tap_mode = MVD_TAPS_CENTRE_TAIL): the algebra that lets a ResBlock's conv2 carry its
1x1 skip convolution as extra k-tiles, checked in float64 on the CPU -- the k-tile order of hip.tap_schedule is the order the kernels walk
(csrc/gemm_device.hpp: conv_tail_start) and the order hip.pack_conv3x3_tail lays the weight out in."""
import pytest
import torch
import torch.nn.functional as F

from mvdfusion_amd import hip


def g(seed):
    return torch.Generator().manual_seed(seed)


def _gemm_in_schedule_order(a, x, w, wt, sched):
    """out (B, H, W, Cout) = sum over the schedule's k-tiles of [32 channels of operand `src` shifted by the tap] @ [that weight block]^T."""
    B, Ca, H, W = a.shape
    ops = (F.pad(a, (1, 1, 1, 1)), F.pad(x, (1, 1, 1, 1)))
    out = torch.zeros(B, H, W, w.shape[0], dtype=torch.float64)
    for src, cb, tap in sched:
        ky, kx = divmod(tap, 3)
        blk = ops[src][:, cb * 32:(cb + 1) * 32, ky:ky + H, kx:kx + W].permute(0, 2, 3, 1)      # zero padding: rows / columns outside are 0
        wb = w[:, cb * 32:(cb + 1) * 32, ky, kx] if src == 0 else wt[:, cb * 32:(cb + 1) * 32]
        out += blk @ wb.t()
    return out


@pytest.mark.parametrize("B,H,W,Ca,Cx,Co", [(2, 5, 7, 64, 96, 40), (1, 1, 1, 32, 64, 48), (3, 3, 1, 96, 32, 16), (1, 2, 9, 32, 160, 33)])
def test_conv_plus_centre_tap_tail_is_conv2_plus_skip(B, H, W, Ca, Cx, Co):
    """[W2 | Wsk] over [im2col(a2) | x] with bias b2 + bsk == conv2(a2) + conv1x1(x) (openaimodel.py:241,274), odd and non-square sizes."""
    a = torch.randn(B, Ca, H, W, generator=g(1), dtype=torch.float64)
    x = torch.randn(B, Cx, H, W, generator=g(2), dtype=torch.float64)
    w = torch.randn(Co, Ca, 3, 3, generator=g(3), dtype=torch.float64)
    wt = torch.randn(Co, Cx, generator=g(4), dtype=torch.float64)
    b, bt = torch.randn(Co, generator=g(5)), torch.randn(Co, generator=g(6))          # fp32 parameters, as the modules hold them
    ref = F.conv2d(a, w, b.double(), padding=1) + F.conv2d(x, wt[:, :, None, None], bt.double())
    sched = hip.tap_schedule(Ca, Cx)
    assert len(sched) == (9 * Ca + Cx) // 32
    got = _gemm_in_schedule_order(a, x, w, wt, sched) + (b.double() + bt.double())
    assert float((got.permute(0, 3, 1, 2) - ref).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max()))
    # the composed bias is the fp64 sum rounded once
    assert torch.equal(hip.compose_conv_tail_bias(b, bt), (b.double() + bt.double()).float())
    assert torch.equal(hip.compose_conv_tail_bias(None, bt), bt) and hip.compose_conv_tail_bias(None, None) is None


@pytest.mark.parametrize("Ca,Cx", [(64, 96), (32, 32), (320, 960), (1280, 2560)])
def test_schedule_lists_exactly_the_nonzero_blocks(Ca, Cx):
    """conv2(a2) + conv1x1(x) is a 3x3 convolution of [a2 | x] whose weight is zero in every x block except at the centre tap: the schedule
    is the list of its non-zero (32-channel block, tap) weight blocks, each once, in k order."""
    Co = 8
    we = torch.zeros(Co, Ca + Cx, 3, 3)
    we[:, :Ca] = torch.rand(Co, Ca, 3, 3, generator=g(7)) + 0.5
    we[:, Ca:, 1, 1] = torch.rand(Co, Cx, generator=g(8)) + 0.5
    nonzero = {(cb, tap) for cb in range((Ca + Cx) // 32) for tap in range(9)
               if bool(we[:, cb * 32:(cb + 1) * 32, tap // 3, tap % 3].abs().sum() > 0)}
    sched = hip.tap_schedule(Ca, Cx)
    listed = [(cb if src == 0 else Ca // 32 + cb, tap) for src, cb, tap in sched]
    assert len(listed) == len(set(listed)) == len(nonzero) and set(listed) == nonzero
    assert sched[:9] == [(0, 0, t) for t in range(9)] and sched[9 * (Ca // 32):] == [(1, cb, 4) for cb in range(Cx // 32)]
    assert hip.tap_schedule(Ca) == [(0, cb, t) for cb in range(Ca // 32) for t in range(9)]          # no tail: the plain nine-tap walk


def test_descriptor_mirror_carries_the_tap_schedule_fields():
    names = [f[0] for f in hip.GemmDesc._fields_]
    assert names[-4:] == ["tap_mode", "A2", "lda2", "Cin2"]          # additive: appended behind the existing fields
    assert (hip.TAPS_FULL, hip.TAPS_CENTRE_TAIL) == (0, 2)
