"""Float64 reference of the GridAttn token kernels (mvd_gridattn_tokens* and mvd_gridattn_tokens_backward*) -- TEST INFRASTRUCTURE.

Takes the arguments of the C entry points (include/mvd_hip.h) as the fp32 tensors the kernels receive, casts them up and evaluates
oracle/ref_torch.gridattn_tokens -- the plain-torch restatement of the operation, pinned against the reference by the fixtures under
tests/golden -- in `dtype` (float64: the reference; float32: the "fp32 oracle" whose own error against float64 sizes the bounds of
tests/test_gpu_gridattn_f64.py).  What this module adds to the oracle is only what the C ABI adds: step rows, scenes, query-view shards,
the window's slot -> view rule and the kernel's row order ((scene, query view, pixel, depth sample), slot).

Also here: the camera rigs of those tests (the GSO rig, a general rig, either with every length scaled) and the bookkeeping of the
exclusion rule (camera-space z of every (point, camera) pair).  Everything runs on the CPU.
"""
import math
from dataclasses import dataclass

import torch

from mvdfusion_amd import synthetic as syn
from mvdfusion_amd.cameras import Cameras, get_camera_slice, get_relative_camera, pack_cameras
from oracle import ref_torch as O

# column families of a token row (include/mvd_hip.h; view_attn_efficient2.py:364-370)
FAMILIES = (("ref samples", 0, 256), ("input samples", 256, 512), ("ref Plucker", 512, 602), ("ref distance", 602, 617),
            ("query Plucker", 617, 707), ("query depth", 707, 722))
MARGIN = 4.0          # kernel and fp32 oracle are two fp32 evaluation orders of the same formulas (with different sin / cos)
Z_EXCLUDE = 0.1       # a (point, camera) pair with |z| < Z_EXCLUDE * rig distance is ill-conditioned: left out
MAX_EXCLUDED = 0.01   # ... and at most this share of the pairs of a case may be


def window_view(b, j, W, V):
    """Slot j of query view b with a window of W slots on a V-view rig (include/mvd_hip.h, mvd_gridattn_tokens_window)."""
    return (b + j - W // 2) % V


def slot_views(V, q0, Vq, window):
    """(Vq, slots) long: the view every slot of every query view of the shard [q0, q0 + Vq) reads; all V views in order without a window."""
    W = window or V
    return torch.tensor([[window_view(b, j, W, V) if window else j for j in range(W)] for b in range(q0, q0 + Vq)], dtype=torch.long)


def step_rows(ts):
    """Step-table rows (MVD_STEP_STRIDE floats each) of timesteps ts: [t, sqrt(alpha_bar), depth std, ...] in fp32."""
    from mvdfusion_amd.scheduler import make_tables
    tab = make_tables()
    rows = []
    for t in ts:
        sac = tab["sqrt_alphas_cumprod"][t]
        rows.append([float(t), float(sac), float(tab["sqrt_one_minus_alphas_cumprod"][t] / sac / 10.0), 1.0, 1.0, 0.0, 0.0, 0.0])
    return torch.tensor(rows, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ rigs
RIG_DISTANCE = 1.5


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
    ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
    return rx @ ry @ rz


def make_rig(V, general, seed=0, length_scale=1.0):
    """(batch cameras (V), input camera (1)): the GSO views the model's own inputs use (synthetic.make_inputs), and with `general` per
    view: fy ~ 1.3 fx with +-20 % focal jitter, principal points up to +-0.15, an extra rotation of up to 0.15 rad per axis (composed in
    float64 from exact rotations, so orthonormal to fp32 rounding) and +-0.1 translation jitter.  length_scale multiplies the translations
    (the caller scales depth_scale / depth_shift with it: the same scene in other units)."""
    rig = get_relative_camera(syn.gso_rig(), [0])
    in_idx, b_idx = syn.select_views(16, V)
    cams = get_camera_slice(rig, torch.cat([b_idx, in_idx]))
    n = V + 1
    R, T, f, p = cams.R.double(), cams.T.double(), cams.focal_length.double(), cams.principal_point.double()
    if general:
        g = torch.Generator().manual_seed(7700 + seed)
        u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1
        fx = f[:, 0] * (1 + 0.2 * u(n))
        f = torch.stack([fx, 1.3 * fx * (1 + 0.05 * u(n))], dim=1)
        p = 0.15 * u(n, 2)
        ang = 0.15 * u(n, 3)
        R = torch.stack([R[i] @ _rot(*ang[i].tolist()) for i in range(n)])
        T = T + 0.1 * u(n, 3)
    T = T * length_scale
    c = Cameras(R.float(), T.float(), f.float(), p.float())
    return get_camera_slice(c, list(range(V))), get_camera_slice(c, [V])


@dataclass
class Case:
    """The arguments of one launch, as the fp32 CPU tensors the kernels receive (layouts: include/mvd_hip.h)."""
    x: torch.Tensor
    depth_noise: torch.Tensor
    steps: torch.Tensor
    cams: Cameras
    in_cam: Cameras
    feat: torch.Tensor
    in_feat: torch.Tensor
    V: int
    q0: int
    Vq: int
    S: int
    D: int
    depth_scale: float
    depth_shift: float
    nscene: int = 1
    steps_scene_stride: int = 0
    window: int = 0
    it: int = 0
    distance: float = RIG_DISTANCE

    @property
    def slots(self):
        return self.window or self.V

    @property
    def npts(self):
        return self.nscene * self.Vq * self.S * self.S * self.D

    def packed(self):
        return pack_cameras(self.cams), pack_cameras(self.in_cam)


def make_case(V, S, D, general, ts, seed, length_scale=1.0, q0=0, Vq=None, window=0, per_scene_steps=False):
    """A case on `len(ts)` scenes when per_scene_steps (a step row and a rig per scene), else one scene at timestep ts[0]: x = 0.5 N(0, 1)
    (with timesteps near 1000 most depth samples clip, near 0 few do), N(0, 1) feature maps and depth noise."""
    N = len(ts) if per_scene_steps else 1
    g = torch.Generator().manual_seed(4100 + seed)
    rigs = [make_rig(V, general, seed + 31 * n, length_scale) for n in range(N)]
    cat = lambda cs: Cameras(*(torch.cat([getattr(c, k) for c in cs]) for k in ("R", "T", "focal_length", "principal_point")))
    return Case(x=torch.randn(N * V, 5, S, S, generator=g) * 0.5, depth_noise=torch.randn(1, N * V, D, S, S, generator=g),
                steps=step_rows(ts), cams=cat([r[0] for r in rigs]), in_cam=cat([r[1] for r in rigs]),
                feat=torch.randn(N * V, S, S, 256, generator=g), in_feat=torch.randn(N, S, S, 256, generator=g), V=V, q0=q0,
                Vq=V if Vq is None else Vq, S=S, D=D, depth_scale=2.0 * length_scale, depth_shift=0.5 * length_scale, nscene=N,
                steps_scene_stride=1 if per_scene_steps else 0, window=window, distance=RIG_DISTANCE * length_scale)


# ------------------------------------------------------------------------------------------------ the reference
@dataclass
class Ref:
    tokens: torch.Tensor          # (T, 723): row (point, slot), points ordered (scene, query view, pixel, depth sample)
    dfeat: torch.Tensor           # (nscene * V, S, S, 256) gradient of sum(tokens * dtok) w.r.t. feat; None without dtok
    din_feat: torch.Tensor        # (nscene, S, S, 256)
    z_ref: torch.Tensor           # (npts, slots) float64: camera-space z of the point in its slot's view
    z_in: torch.Tensor            # (npts,) ... in its scene's input view
    outside: float                # share of the (point, slot view) projections outside the image (|ndc| > 1 on either axis), float64


def _cam_dict(c, sl, dtype):
    return {"R": c.R[sl].to(dtype), "T": c.T[sl].to(dtype), "f": c.focal_length[sl].to(dtype), "p": c.principal_point[sl].to(dtype)}


def depth_samples(case, n, dtype=torch.float64):
    """(V, D, S, S) metric depth samples of scene n, as O.gridattn_forward draws them, from the fp32 step row of the scene."""
    V = case.V
    row = case.steps[case.it + n * case.steps_scene_stride].to(dtype)
    sac, dstd = row[1], row[2]
    dch = case.x[n * V:(n + 1) * V, 4:].to(dtype) / sac
    smp = dch + dstd * case.depth_noise[case.it, n * V:(n + 1) * V].to(dtype)
    return torch.clip((smp + 1.0) / 2.0, 0.0, 1.0) * case.depth_scale + case.depth_shift


def world_points(cams, depth, S):
    """(V, S*S*D, 3): the 3-D points O.gridattn_tokens builds (same calls; it does not return them), for the z bookkeeping."""
    V, D = depth.shape[:2]
    R, T, f, p = cams["R"], cams["T"], cams["f"], cams["p"]
    lin = torch.linspace(1.0 - 1.0 / S, -1.0 + 1.0 / S, S, dtype=torch.float32).to(R.dtype)
    yy, xx = torch.meshgrid(lin, lin, indexing="ij")
    xy = torch.stack([xx, yy], dim=-1).reshape(1, S * S, 2).expand(V, -1, -1)
    ones = torch.ones(V, S * S, dtype=R.dtype)
    p1 = O.unproject_ndc(R, T, f, p, xy, ones)
    dirs = O.unproject_ndc(R, T, f, p, xy, 2.0 * ones) - p1
    lengths = depth.permute(0, 2, 3, 1).reshape(V, S * S, D)
    return ((p1 - dirs)[:, :, None, :] + lengths[..., None] * dirs[:, :, None, :]).reshape(V, S * S * D, 3)


def reference(case, dtok=None, dtype=torch.float64):
    """The token matrix of `case` in the kernel's row order, the gradients of sum(tokens * dtok[:, :723]) w.r.t. feat / in_feat by autograd
    through O.gridattn_tokens (dtok (T, >= 512); None: no gradients), and the z bookkeeping -- all evaluated in `dtype`."""
    V, S, D, q0, Vq = case.V, case.S, case.D, case.q0, case.Vq
    views = slot_views(V, q0, Vq, case.window)                                     # (Vq, W)
    W = views.shape[1]
    feat = case.feat.to(dtype).requires_grad_(dtok is not None)
    in_feat = case.in_feat.to(dtype).requires_grad_(dtok is not None)
    toks, z_ref, z_in, outside = [], [], [], []
    for n in range(case.nscene):
        sl = slice(n * V, (n + 1) * V)
        cams, in_cam = _cam_dict(case.cams, sl, dtype), _cam_dict(case.in_cam, slice(n, n + 1), dtype)
        depth = depth_samples(case, n, dtype)
        z = O.gridattn_tokens(feat[sl].permute(0, 3, 1, 2), in_feat[n:n + 1].permute(0, 3, 1, 2), cams, in_cam, depth, S)
        z = z.permute(1, 2, 0, 3)[q0:q0 + Vq]                                      # (query view, pixel * D + d, reference view, 723)
        toks.append(torch.stack([z[i][:, views[i]] for i in range(Vq)]))         # (Vq, S*S*D, W, 723)
        with torch.no_grad():
            pts = world_points(cams, depth, S)[q0:q0 + Vq]                         # (Vq, n, 3)
            ndc = O.project_ndc(cams["R"], cams["T"], cams["f"], cams["p"], pts.reshape(-1, 3))          # (V, Vq*n, 3): (u, v, 1/z)
            ndc = ndc.reshape(V, Vq, -1, 3).permute(1, 2, 0, 3)                    # (Vq, n, V, 3)
            ndc = torch.stack([ndc[i][:, views[i]] for i in range(Vq)])          # (Vq, n, W, 3)
            z_ref.append((1.0 / ndc[..., 2]).reshape(-1, W))
            outside.append((ndc[..., :2].abs() > 1.0).any(-1).reshape(-1, W))
            ndi = O.project_ndc(in_cam["R"], in_cam["T"], in_cam["f"], in_cam["p"], pts.reshape(-1, 3))
            z_in.append((1.0 / ndi[0, :, 2]).reshape(-1))
    tokens = torch.cat(toks).reshape(-1, 723)
    dfeat = din_feat = None
    if dtok is not None:
        k = min(dtok.shape[1], 723)
        dfeat, din_feat = torch.autograd.grad((tokens[:, :k] * dtok[:, :k].to(dtype)).sum(), [feat, in_feat])
    return Ref(tokens.detach(), dfeat, din_feat, torch.cat(z_ref).double(), torch.cat(z_in).double(),
               float(torch.cat(outside).double().mean()))


# ------------------------------------------------------------------------------------------------ the exclusion rule
def excluded(case, ref):
    """(bad_ref (npts, slots), bad_in (npts,)) bool: the (point, camera) pairs left out, from the FLOAT64 z; asserts the cap."""
    lim = Z_EXCLUDE * case.distance
    bad_ref, bad_in = ref.z_ref.abs() < lim, ref.z_in.abs() < lim
    share = float(bad_ref.sum() + bad_in.sum()) / float(bad_ref.numel() + bad_in.numel())
    assert share <= MAX_EXCLUDED, f"{share:.2%} of the (point, camera) pairs are ill-conditioned (cap {MAX_EXCLUDED:.0%})"
    return bad_ref, bad_in


def family_rows(fam, bad_ref, bad_in):
    """(T,) bool: the token rows kept for column family `fam`: an excluded input-view pair removes the point's rows (from every family),
    an excluded reference pair its row's sample columns."""
    keep = (~bad_in)[:, None].expand_as(bad_ref)
    if fam == "ref samples":
        keep = keep & ~bad_ref
    return keep.reshape(-1)


def zero_excluded(dtok, bad_ref, bad_in):
    """dtok (T, ldt) with the rows of excluded pairs zeroed in place: they then contribute nothing to either implementation's gradient."""
    W = bad_ref.shape[1]
    d = dtok.view(-1, W, dtok.shape[1])
    d[:, :, :256] *= (~bad_ref)[:, :, None].to(d.dtype)
    d[:, :, 256:512] *= (~bad_in)[:, None, None].to(d.dtype)
    return dtok
