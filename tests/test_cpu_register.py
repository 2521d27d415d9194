"""The global registration without a GPU: header, binding and constants; fusion.rotation_grid against its restatement and the covering
radii; the float64 oracle of tests/register_f64.py on the pose table at fusion's defaults -- the condition that keeps
tests/test_gpu_register.py honest: what the GPU is asked to recover, the reference recovers -- and the oracle's plain centroid ICP on the
same poses, which does not; the host side of fusion.register_geometry against stub enqueues."""
import math
import os
import re

import numpy as np
import pytest
import torch

import align_f64 as A
import register_f64 as RG
from mvdfusion_amd import fusion, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ICP_BOUND = 2.0 ** -20           # tests/test_gpu_align.py has the derivation: the fp32 rounding of both point sets
GPU_POSES = RG.GPU_POSES


# ------------------------------------------------------------------------------------------------ header, binding, constants
def test_the_header_and_the_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+MVD_REGISTER_(\w+)\s+(\d+)", hdr)}
    assert consts == dict(MAX_H=hip.REGISTER_MAX_H, MAX_K=hip.REGISTER_MAX_K) and consts == dict(MAX_H=16384, MAX_K=32)
    for name, count in (("mvd_register_scratch", 6), ("mvd_register_score", 17), ("mvd_register_select", 9)):
        decl = re.search(r"^\w+ " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl is not None and name in hip.SIGNATURES, name
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == count, name
    build = open(os.path.join(ROOT, "mvdfusion_amd", "csrc", "build.py")).read()
    assert '"register.hip"' in build and '"nn_points.hpp"' in build and '"align_common.hpp"' in build
    src = open(os.path.join(ROOT, "mvdfusion_amd", "csrc", "register.hip")).read()
    assert "atomic" not in src.split('#include "nn_points.hpp"')[1] and "nn_walk_grid(" in src and "al_apply(" in src      # no atomics; THE walk, THE apply
    L = hip.lib()
    nn = int(L.mvd_nearest_points_scratch(5000, 2, hip.NN_GRID, 7))
    need = int(L.mvd_register_scratch(3000, 5000, 2, 65, hip.NN_GRID, 7))
    assert need >= nn + (3 + 2) * 65 * 12 + 3 * 4              # the grid, a double and an int per (chunk, h), the chunk map
    assert int(L.mvd_register_scratch(3000, 5000, 2, 65, hip.NN_BRUTE, 0)) == need - nn
    for args in ((10, 10, 0, 1, 0, 0), (10, 10, 65536, 1, 0, 0), (10, 10, 1, 0, 0, 0), (10, 10, 1, hip.REGISTER_MAX_H + 1, 0, 0),
                 (10, 10, 1, 1, 3, 0), (10, 10, 1, 1, 0, 257), (1 << 31, 10, 1, 1, 0, 0), (10, 1 << 31, 1, 1, 0, 0),
                 (10, 10, 65535, 1, hip.NN_GRID, 256)):
        assert int(L.mvd_register_scratch(*args)) == 0, args
    d = RG.DEFAULTS
    assert (fusion.REGISTER_ROTATIONS, fusion.REGISTER_SAMPLES, fusion.REGISTER_CANDIDATES, fusion.ALIGN_ITERS) == (d["H"], d["samples"], d["K"], d["iters"])
    assert "no global registration" not in fusion.align_geometry.__doc__ and "register_geometry" in fusion.align_geometry.__doc__


# ------------------------------------------------------------------------------------------------ the rotation grid
def test_rotation_grid_is_the_spiral_unit_and_deterministic():
    for H in (1, 7, 256, 4096):
        q = fusion.rotation_grid(H)
        assert q.dtype == torch.float64 and tuple(q.shape) == (H, 4)
        assert float((q.norm(dim=1) - 1).abs().max()) <= 4 * 2.0 ** -53
        assert np.array_equal(q.numpy(), RG.rotation_grid(H)) and torch.equal(q, fusion.rotation_grid(H))
    R = fusion._quat_matrix(fusion.rotation_grid(64))
    assert np.abs(R.numpy() - RG.quat_matrix(RG.rotation_grid(64))).max() <= 8 * 2.0 ** -53
    back = fusion._matrix_quat(R)
    assert float(RG.angle_between(back.numpy(), RG.rotation_grid(64)).max()) <= 1e-5
    for bad in (0, hip.REGISTER_MAX_H + 1, 2.5, True, "8"):
        with pytest.raises(ValueError):
            fusion.rotation_grid(bad)


@pytest.mark.parametrize("H, quoted", [(256, 35.0), (1024, 20.0), (4096, 13.0)])
def test_the_covering_radius_of_the_grid(H, quoted):
    got = RG.covering_radius(H)
    print(f"RATIO register covering radius H {H}: {got:.2f} degrees (quoted {quoted})")
    assert abs(got - quoted) <= 0.1 * quoted


# ------------------------------------------------------------------------------------------------ the oracle on the pose table
@pytest.mark.parametrize("k", range(len(RG.pose_table())))
def test_the_oracle_recovers_every_pose_at_the_defaults(k):
    case = RG.pose_case(k)
    ref = RG.register_ref(k)
    order = np.sort(ref.candidate_score)
    print(f"RATIO register oracle pose {k} ({RG.pose_angle(k):.1f} deg) | |M - truth| {ref.error:.2e} right {ref.right}/{case.n} | "
          f"chosen {ref.chosen} score {order[0]:.2e} next {order[1]:.2e} | candidate errors {np.array2string(ref.candidate_error, precision=1)}")
    assert ref.error <= ICP_BOUND and ref.right == case.n
    assert ref.candidate_score[ref.chosen] == order[0]


def test_the_oracles_plain_centroid_icp_does_not_recover_them():
    """What the feature is for: ICP from init="centroid" on the same inputs ends in a flipped basin."""
    missed = 0
    for k in range(len(RG.pose_table())):
        err = RG.centroid_icp_error(k)
        missed += err > 0.5
        print(f"RATIO register oracle pose {k} ({RG.pose_angle(k):.1f} deg): centroid ICP ends at |M - truth| {err:.2e}")
    print(f"RATIO register: centroid ICP misses {missed} of {len(RG.pose_table())} poses")
    for k in GPU_POSES:
        assert RG.centroid_icp_error(k) > 0.5, k


def test_select_in_the_oracle_is_the_greedy_rule():
    q = RG.rotation_grid(64)
    score = np.linspace(1.0, 2.0, 64)
    score[[5, 9]] = [0.5, 0.5]
    score[3] = float("nan")
    top, top_score = RG.select(score, q, 2.0, 4)
    assert top.tolist() == [5, 9, 0, 1] and top_score.tolist() == [0.5, 0.5, score[0], score[1]]
    top, _ = RG.select(score, q, math.cos(math.radians(60.0) / 2), 64)
    taken = top[top >= 0]
    assert 3 not in taken and len(taken) < 64 and (top[len(taken):] == -1).all()
    ang = RG.angle_between(q[taken][:, None], q[taken][None]) + 1e3 * np.eye(len(taken))
    assert ang.min() > 60.0


# ------------------------------------------------------------------------------------------------ the host side
def _mesh():
    return fusion.TriangleMesh(vertices=torch.rand(3, 3), faces=torch.tensor([[0, 1, 2]], dtype=torch.int32), rgb=None,
                               vertex_start=torch.tensor([0, 3], dtype=torch.int32), face_start=torch.tensor([0, 1], dtype=torch.int32))


def test_register_geometry_validates_before_it_reaches_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(hip, "lib", no_library)
    a, b = torch.rand(50, 3), torch.rand(60, 3)
    bad = [dict(scenes=0), dict(rotations=0), dict(rotations=hip.REGISTER_MAX_H + 1), dict(rotations=torch.zeros(3, 5)),
           dict(rotations=torch.zeros(2, 4)), dict(rotations=torch.full((1, 4), float("nan"))), dict(rotations=-torch.eye(3)[None]),
           dict(samples=0), dict(samples=1.5), dict(candidates=0), dict(candidates=hip.REGISTER_MAX_K + 1), dict(separation=-1.0),
           dict(separation=181.0), dict(trunc=0.0), dict(trunc=float("inf")), dict(trunc=float("nan")), dict(scale=1), dict(refine_iters=-1),
           dict(iters=hip.ALIGN_MAX_ITERS + 1), dict(max_distance=-1.0), dict(method="tree"), dict(grid=0), dict(source=torch.rand(5, 2)),
           dict(trunc=1e-30)]
    for kw in bad:
        args = dict(source=a, target=b)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.register_geometry(**args)
    with pytest.raises(ValueError, match="a TriangleMesh has no points to search"):
        fusion.register_geometry(a, _mesh())
    with pytest.raises(ValueError, match="trunc = None"):
        fusion.register_geometry(a, torch.zeros(0, 3))
    for text in ("INTERFACE defaults", "sample_mesh(mesh, n)", "partial"):
        assert text in fusion.register_geometry.__doc__, text


@pytest.fixture
def stub(monkeypatch):
    calls = []

    def build(target, target_start, N, method, grid, scratch, nbytes):
        calls.append(dict(fn="build", nbytes=nbytes))

    def score(points, start, target, target_start, N, hyp, trunc2, method, grid, scratch, nbytes):
        calls.append(dict(fn="score", points=points, start=start, hyp=hyp.clone(), trunc2=trunc2))
        H = hyp.shape[1]
        return torch.arange(N * H, dtype=torch.float64).reshape(N, H).flip(1), torch.zeros(N, H, dtype=torch.int32)

    def select(score, quat, K, cos_half):
        calls.append(dict(fn="select", K=K, cos_half=cos_half, H=int(score.shape[1])))
        order = torch.argsort(score, dim=1)[:, :K].to(torch.int32)
        return order, torch.gather(score, 1, order.long())

    def icp(source, source_start, target, target_start, N, method, grid, iters, flags, max_d2, transform):
        calls.append(dict(fn="icp", iters=iters, flags=flags, max_d2=max_d2, start=transform.clone(), n=int(source.shape[0])))
        history = torch.ones(iters + 1, N, 3, dtype=torch.float64)
        return history, source.clone(), torch.zeros(source.shape[0], dtype=torch.int32), torch.zeros(source.shape[0])

    monkeypatch.setattr(fusion, "_register_scratch", lambda *a: 64)
    monkeypatch.setattr(fusion, "_register_build", build)
    monkeypatch.setattr(fusion, "_register_score", score)
    monkeypatch.setattr(fusion, "_register_select", select)
    monkeypatch.setattr(fusion, "_align_icp", icp)
    return calls


def test_register_geometry_forms_the_hypotheses_and_the_sequence(stub):
    case = RG.pose_case(0)
    reg = fusion.register_geometry(case.source, case.target, rotations=16, samples=100, candidates=3, refine_iters=5, iters=7)
    assert [c["fn"] for c in stub] == ["build", "score", "select", "icp", "icp", "icp", "score", "select", "icp"]
    first, sel, second, sel1 = stub[1], stub[2], stub[6], stub[7]
    want = RG.hypotheses(RG.quat_matrix(RG.rotation_grid(16)), case.source, case.target)
    assert np.abs(first["hyp"].numpy().reshape(16, 3, 4) - want).max() <= 16 * 2.0 ** -53
    rows = RG.sample_rows(case.n, 100)
    assert torch.equal(first["points"], case.source[torch.from_numpy(rows)]) and first["start"].tolist() == [0, len(rows)] and len(rows) <= 100
    _, r2 = RG.centroid_stats(case.target)
    t = np.float32(0.1 * math.sqrt(r2))
    assert first["trunc2"] == float(np.float32(t * t)) == second["trunc2"]
    assert sel["K"] == 3 and sel["H"] == 16 and abs(sel["cos_half"] - math.cos(math.radians(15.0))) <= 1e-15
    assert sel1["K"] == 1 and sel1["H"] == 3 and sel1["cos_half"] > 1
    assert [c["iters"] for c in stub if c["fn"] == "icp"] == [5, 5, 5, 7] and all(c["n"] == case.n for c in stub if c["fn"] == "icp")
    # the stub scores fall with h: the three refined are hypotheses 15, 14, 13, and the last (lowest) refined score is chosen
    for k, c in enumerate(stub[3:6]):
        assert np.abs(c["start"].numpy().reshape(3, 4) - want[15 - k]).max() <= 16 * 2.0 ** -53
    assert tuple(second["hyp"].shape) == (1, 3, 12) and second["points"].shape[0] == case.n
    assert reg.chosen.tolist() == [2] and isinstance(reg, fusion.Alignment)
    assert tuple(reg.candidates.shape) == (1, 3, 4, 4) and tuple(reg.grid_score.shape) == (1, 16) and tuple(reg.rms.shape) == (8, 1)
    assert torch.equal(reg.candidates[0, :, 3], torch.tensor([[0.0, 0.0, 0.0, 1.0]] * 3, dtype=torch.float64))
    assert torch.equal(reg.matrix[0, :3], reg.candidates[0, 2, :3])
    # given rotations: the identity alone is init="centroid"
    stub.clear()
    fusion.register_geometry(case.source, case.target, rotations=torch.eye(3)[None], candidates=1, separation=0.0, trunc=0.05)
    cen = RG.hypotheses(np.eye(3)[None], case.source, case.target)
    assert np.abs(stub[1]["hyp"].numpy().reshape(1, 3, 4) - cen).max() <= 16 * 2.0 ** -53 and stub[2]["cos_half"] > 1
    t = np.float32(0.05)
    assert stub[1]["trunc2"] == float(np.float32(t * t))
