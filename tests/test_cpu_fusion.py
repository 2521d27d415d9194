"""View fusion without a GPU: the float64 reference of tests/fusion_f64.py against the geometry that is already pinned to the real
reference (gridattn_f64.world_points), its known answer on a sphere, the exclusion cap of every parity case of tests/test_gpu_fusion.py,
and the host side of mvdfusion_amd/fusion.py (argument validation and the rgb resize rule with the two launches stubbed; write_ply)."""
import functools

import numpy as np
import pytest
import torch

import fusion_f64 as F
import gridattn_f64 as G
from mvdfusion_amd import fusion
from mvdfusion_amd.cameras import get_camera_slice


@functools.lru_cache(maxsize=None)
def _refs(name):
    case = F.make_case(name)
    return case, F.reference(case), F.reference(case, torch.float32)


@functools.lru_cache(maxsize=None)
def _sphere(pull_view=None):
    case = F.sphere_case(pull_view=pull_view)
    return case, F.reference(case)


def test_reference_world_points_are_the_gridattn_world_points():
    """up = 1: the fusion reference unprojects (ndc, z) directly, GridAttn walks origin + z * direction of the same ray -- the same points
    in float64 to 1e-12, for the same metric depths."""
    case, ref, _ = _refs("general_v5_s12")
    depth = F.metric_depth(case, torch.float64)[:, None]
    want = G.world_points(G._cam_dict(case.cams, slice(0, case.V), torch.float64), depth, case.S).reshape(-1, 3)
    assert ref.xyz.shape == want.shape
    assert float((ref.xyz - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", list(F.CASES))
def test_parity_cases_respect_the_exclusion_cap(name):
    """... and are worth running: foreground and background taps both occur, votes of both kinds are cast, and the fp32 oracle agrees with
    float64 on every compared point (so the counts CAN be asserted equal)."""
    case, ref, o32 = _refs(name)
    bad, m_z, m_n = F.undecidable(case, ref, o32)          # asserts the cap
    keep = F.compared_points(bad)
    share = float(ref.fg.float().mean())
    print(f"{name}: foreground {share:.3f}, undecidable pairs {float(bad.sum()) / max(1, int(ref.other.sum())):.2%}, m_z {m_z:.1e}, "
          f"m_n {m_n:.1e}, fp32 oracle xyz {float((o32.xyz.double() - ref.xyz).abs().max()):.1e}")
    assert 0.9 <= share < 1.0
    assert torch.equal(o32.fg, ref.fg)
    assert torch.equal(o32.support[keep], ref.support[keep]) and torch.equal(o32.conflict[keep], ref.conflict[keep])
    assert float((o32.xyz.double() - ref.xyz).abs().max()) <= 4e-7
    if case.V == 1:
        assert int(ref.support.sum()) == 0 and int(ref.conflict.sum()) == 0
    else:
        assert int(ref.support.sum()) > 0 and int(ref.conflict.sum()) > 0 and bool((~ref.votes & ref.other).any())


def test_sphere_known_answer_float64():
    case, ref = _sphere()
    V, n = case.V, case.P * case.P
    fg, keep = ref.fg.reshape(V, n), F.kept(ref).reshape(V, n)
    assert int(ref.conflict.sum()) == 0
    assert fg.sum(1).tolist() == [732] * V and keep.sum(1).tolist() == [696] * V          # 0.951 of the foreground in every view
    assert float((ref.xyz[ref.fg].norm(dim=1) - F.SPHERE_R).abs().max()) <= 3e-8


def test_sphere_with_one_view_pulled_forward_float64():
    """View 1's surface 0.3 nearer its camera: nothing supports it, the views that do not border it keep exactly what they kept, the two
    neighbours lose the points view 1 now contradicts."""
    case, ref = _sphere()
    case2, ref2 = _sphere(1)
    V, n = case.V, case.P * case.P
    keep, keep2 = F.kept(ref).reshape(V, n), F.kept(ref2).reshape(V, n)
    assert int(keep2[1].sum()) == 0 and int(ref2.support.reshape(V, n)[1][ref2.fg.reshape(V, n)[1]].max()) == 0
    for v in (3, 4, 5, 6, 7):
        assert torch.equal(keep2[v], keep[v]), v
    for v in (0, 2):
        assert bool((keep2[v] <= keep[v]).all()) and int(keep2[v].sum()) < int(keep[v].sum()), v


# ------------------------------------------------------------------------------------------------ host
def _stub(monkeypatch):
    calls = []

    def run(lat, rgb, cams, N, V, S, up, depth_scale, depth_shift, lo, hi, tau, min_support, max_conflicts):
        calls.append(dict(lat=lat, rgb=rgb, cams=cams, N=N, V=V, S=S, up=up, depth_scale=depth_scale, depth_shift=depth_shift, lo=lo, hi=hi,
                          tau=tau, min_support=min_support, max_conflicts=max_conflicts))
        P = S * up
        index = torch.tensor([0, P + 1, N * V * P * P - 1], dtype=torch.int32)
        return torch.zeros(3, 3), None if rgb is None else torch.zeros(3, 3), torch.ones(3, dtype=torch.uint8), index

    monkeypatch.setattr(fusion, "_run", run)
    return calls


def test_fuse_views_validates_its_arguments(monkeypatch):
    calls = _stub(monkeypatch)
    V, S = 3, 8
    cams = G.make_rig(V, True)[0]
    lat = torch.zeros(V, 5, S, S)
    bad = [
        dict(latents=lat[:, :4]), dict(latents=lat[0]), dict(latents=lat[:, :, :, :7]), dict(latents=lat[:, :, :1, :1]),
        dict(cameras=[cams]), dict(cameras=get_camera_slice(cams, [0, 1])), dict(up=0), dict(up=1.5), dict(tau=-1.0), dict(tau=float("nan")),
        dict(foreground=(0.5, 0.5)), dict(min_support=-1), dict(max_conflicts=256), dict(rgb=torch.zeros(V, 3, 4, 4)),
        dict(rgb=torch.zeros(V, 3, 16, 16), up=4), dict(rgb=torch.zeros(V, 4, 16, 16)), dict(rgb=torch.zeros(V + 1, 3, 16, 16)),
        dict(rgb=torch.zeros(V, 3, 16, 8)), dict(latents=lat[None], cameras=cams), dict(latents=lat[None].expand(2, -1, -1, -1, -1), cameras=[cams]),
        dict(latents=torch.zeros(256, 5, 2, 2), cameras=get_camera_slice(cams, [0] * 256)), dict(up=2 ** 13),
    ]
    for kw in bad:
        args = dict(latents=lat, cameras=cams)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.fuse_views(**args)
    assert not calls                              # nothing reached the library
    pc = fusion.fuse_views(lat, cams)             # the defaults, as documented
    c = calls[-1]
    assert (c["N"], c["V"], c["S"], c["up"]) == (1, V, S, 1) and c["rgb"] is None and c["cams"].shape == (V, 20)
    assert (c["lo"], c["hi"], c["min_support"], c["max_conflicts"]) == (0.02, 0.98, 1, 0)
    assert (c["depth_scale"], c["depth_shift"]) == (2.0, 0.5) and c["tau"] == 0.025 * 2.0
    assert fusion.fuse_views(lat, cams, depth_scale=4.0) is not None and calls[-1]["tau"] == 0.1
    assert len(pc) == 3 and pc.rgb is None


def test_fuse_views_resizes_rgb_and_decodes_the_point_index(monkeypatch):
    calls = _stub(monkeypatch)
    N, V, S, up = 2, 3, 8, 2
    P = S * up
    cams = [G.make_rig(V, True, seed=n)[0] for n in range(N)]
    lat = torch.randn(N, V, 5, S, S)
    rgb = torch.rand(N, V, 3, 4 * P, 4 * P, generator=torch.Generator().manual_seed(1))
    pc = fusion.fuse_views(lat, cams, rgb=rgb, up=up)
    c = calls[-1]
    assert (c["N"], c["V"], c["up"]) == (N, V, up) and c["lat"].shape == (N * V, 5, S, S) and c["cams"].shape == (N * V, 20)
    assert torch.equal(c["rgb"], torch.nn.functional.interpolate(rgb.reshape(N * V, 3, 4 * P, 4 * P), scale_factor=0.25, mode="area"))
    exact = rgb[:, :, :, :P, :P].contiguous()
    fusion.fuse_views(lat, cams, rgb=exact, up=up)
    assert torch.equal(calls[-1]["rgb"], exact.reshape(N * V, 3, P, P))          # H == P: handed on as it is
    assert pc.scene.tolist() == [0, 0, N - 1] and pc.view.tolist() == [0, 0, V - 1]
    assert pc.pixel.tolist() == [[0, 0], [1, 1], [P - 1, P - 1]] and pc.index.tolist() == [0, P + 1, N * V * P * P - 1]
    assert pc.rgb is not None and len(pc) == 3


@pytest.mark.parametrize("colour", [True, False])
def test_write_ply_round_trip(tmp_path, colour):
    g = torch.Generator().manual_seed(3)
    n = 37
    rgb = torch.rand(n, 3, generator=g) if colour else None
    cloud = fusion.PointCloud(xyz=torch.randn(n, 3, generator=g), rgb=rgb, support=torch.ones(n, dtype=torch.uint8),
                              scene=torch.zeros(n, dtype=torch.long), view=torch.zeros(n, dtype=torch.long),
                              pixel=torch.zeros(n, 2, dtype=torch.long), index=torch.arange(n, dtype=torch.int32))
    path = tmp_path / "cloud.ply"
    fusion.write_ply(str(path), cloud)
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").splitlines()
    assert header[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    props = [tuple(line.split()[1:]) for line in header if line.startswith("property")]
    assert props == [("float", "x"), ("float", "y"), ("float", "z")] + ([("uchar", "red"), ("uchar", "green"), ("uchar", "blue")] if colour else [])
    dt = np.dtype([(k, {"float": "<f4", "uchar": "u1"}[t]) for t, k in props])
    v = np.frombuffer(raw[end:], dtype=dt)
    assert v.shape == (n,)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), cloud.xyz.numpy())
    if colour:
        assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), np.rint(rgb.numpy() * 255.0).astype(np.uint8))
