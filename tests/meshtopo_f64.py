"""Integer / float64 numpy restatement of the mesh-topology section of include/mvd_hip.h (csrc/meshtopo.hip): face classes, the
vertex -> (face, corner) incidence table, connected components, the topology report, the face filter, area-weighted vertex normals and
Taubin smoothing.  Not collected by pytest; tests/test_cpu_meshtopo.py holds it to known answers, tests/test_gpu_meshtopo.py holds the
kernels to it.

Components are a plain union-find, edges a dict.  The float64 sums run over the incidence list in list order: the loop is over the
POSITION in the list and vectorised over the vertices, so every vertex adds its terms one at a time in exactly the stated order, each
operation rounded once by numpy's float64, and the single rounding to fp32 is where the header says.
"""
from dataclasses import dataclass

import numpy as np

TOTALS = ("vertices_used", "unreferenced", "faces_regular", "faces_repeated", "faces_invalid", "edges", "boundary_edges",
          "nonmanifold_edges", "misoriented_edges", "components", "euler")
INVALID, REGULAR, REPEATED = -1, 0, 1
FLAG_BOUNDARY, FLAG_NONMANIFOLD = 1, 2


@dataclass
class Mesh:
    vertices: np.ndarray          # (nv, 3) float32
    faces: np.ndarray             # (nf, 3) int32 global ids
    vertex_start: np.ndarray      # (N + 1,) int64
    face_start: np.ndarray
    rgb: np.ndarray = None        # (nv, 3) float32 or None

    @property
    def nscene(self):
        return len(self.face_start) - 1


def make(vertices, faces, vertex_start=None, face_start=None, rgb=None):
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    vs = np.array([0, len(vertices)] if vertex_start is None else vertex_start, dtype=np.int64)
    fs = np.array([0, len(faces)] if face_start is None else face_start, dtype=np.int64)
    return Mesh(vertices, faces, vs, fs, None if rgb is None else np.asarray(rgb, dtype=np.float32).reshape(-1, 3))


def concat(meshes):
    """Scenes one after another with global ids."""
    v0 = np.cumsum([0] + [len(m.vertices) for m in meshes])
    f0 = np.cumsum([0] + [len(m.faces) for m in meshes])
    assert all(m.nscene == 1 for m in meshes)
    rgb = None if meshes[0].rgb is None else np.concatenate([m.rgb for m in meshes])
    return Mesh(np.concatenate([m.vertices for m in meshes]), np.concatenate([m.faces + np.int32(o) for m, o in zip(meshes, v0)]).astype(np.int32),
                v0.astype(np.int64), f0.astype(np.int64), rgb)


def classify(m):
    """(class (nf,), scene (nf,)): INVALID / REGULAR / REPEATED and the face's scene (-1: of no scene)."""
    nf, nv = len(m.faces), len(m.vertices)
    fs, vs = np.clip(m.face_start, 0, nf), np.clip(m.vertex_start, 0, nv)
    f = np.arange(nf)
    scene = np.searchsorted(fs, f, side="right") - 1
    scene = np.where((f >= fs[0]) & (f < fs[-1]), np.minimum(scene, m.nscene - 1), -1)
    s = np.maximum(scene, 0)
    ids = m.faces.astype(np.int64)
    inside = ((ids >= vs[s][:, None]) & (ids < vs[s + 1][:, None])).all(1) & (scene >= 0)
    rep = (ids[:, 0] == ids[:, 1]) | (ids[:, 1] == ids[:, 2]) | (ids[:, 0] == ids[:, 2])
    return np.where(~inside, INVALID, np.where(rep, REPEATED, REGULAR)), scene


def incidence(m):
    """(inc_start (nv + 1,), inc (entries,)): per vertex the entries face * 3 + corner of the regular faces, ascending."""
    cls, _ = classify(m)
    nv = len(m.vertices)
    reg = np.nonzero(cls == REGULAR)[0]
    ent = (reg[:, None] * 3 + np.arange(3)[None, :]).reshape(-1)
    vert = m.faces[reg].astype(np.int64).reshape(-1)
    order = np.lexsort((ent, vert))
    inc_start = np.concatenate([[0], np.cumsum(np.bincount(vert, minlength=nv))]) if nv else np.zeros(1, dtype=np.int64)
    return inc_start.astype(np.int32), ent[order].astype(np.int32)


def components(m):
    cls, scene = classify(m)
    nv, nf = len(m.vertices), len(m.faces)
    parent = list(range(nv))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    used = np.zeros(nv, dtype=bool)
    for f in np.nonzero(cls != INVALID)[0]:
        a, b, c = (int(x) for x in m.faces[f])
        used[[a, b, c]] = True
        for x, y in ((a, b), (a, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    label = np.array([find(v) for v in range(nv)], dtype=np.int64)
    flag = (label == np.arange(nv)) & used
    rank = np.concatenate([[0], np.cumsum(flag)])
    vcomp = np.where(used, rank[label], -1).astype(np.int32) if nv else np.zeros(0, dtype=np.int32)
    fcomp = np.full(nf, -1, dtype=np.int32)
    if nf and nv:
        fcomp = np.where(cls != INVALID, rank[label[np.clip(m.faces[:, 0], 0, nv - 1)]], -1).astype(np.int32)
    ncomp = int(rank[-1])
    cstart = rank[np.clip(m.vertex_start, 0, nv)].astype(np.int32)
    return dict(vertex_component=vcomp, face_component=fcomp, component_start=cstart, root=np.nonzero(flag)[0].astype(np.int32),
                faces=np.bincount(fcomp[fcomp >= 0], minlength=ncomp).astype(np.int32),
                vertices=np.bincount(vcomp[vcomp >= 0], minlength=ncomp).astype(np.int32))


def topology(m):
    """(totals (N, 11) int32 in TOTALS order, vertex_flags (nv,) uint8)."""
    cls, scene = classify(m)
    comp = components(m)
    N, nv = m.nscene, len(m.vertices)
    totals = np.zeros((N, len(TOTALS)), dtype=np.int64)
    flags = np.zeros(nv, dtype=np.uint8)
    vs = np.clip(m.vertex_start, 0, nv)
    edges = [dict() for _ in range(N)]
    for f in range(len(m.faces)):
        s = scene[f]
        if s < 0:
            continue
        if cls[f] != REGULAR:
            totals[s, 4 if cls[f] == INVALID else 3] += 1
            continue
        totals[s, 2] += 1
        ids = [int(x) for x in m.faces[f]]
        for e in range(3):
            a, b = ids[e], ids[(e + 1) % 3]
            edges[s].setdefault((min(a, b), max(a, b)), []).append(a < b)      # the direction the user runs along it
    for s in range(N):
        used = comp["vertex_component"][vs[s]:vs[s + 1]] >= 0
        totals[s, 0], totals[s, 1] = used.sum(), (~used).sum()
        for (a, b), users in edges[s].items():
            totals[s, 5] += 1
            if len(users) == 1:
                totals[s, 6] += 1
                flags[[a, b]] |= FLAG_BOUNDARY
            elif len(users) > 2:
                totals[s, 7] += 1
                flags[[a, b]] |= FLAG_NONMANIFOLD
            elif users[0] == users[1]:
                totals[s, 8] += 1
        totals[s, 9] = comp["component_start"][s + 1] - comp["component_start"][s]
        totals[s, 10] = totals[s, 0] - totals[s, 5] + totals[s, 2]
    return totals.astype(np.int32), flags


def filter_faces(m, keep):
    """The kept faces and the vertices they name -> (Mesh, vertex_index, face_index)."""
    cls, _ = classify(m)
    nv, nf = len(m.vertices), len(m.faces)
    kept = (np.asarray(keep).astype(bool)) & (cls != INVALID)
    vflag = np.zeros(nv, dtype=bool)
    vflag[m.faces[kept].reshape(-1)] = True
    vrank, frank = np.concatenate([[0], np.cumsum(vflag)]), np.concatenate([[0], np.cumsum(kept)])
    out = Mesh(m.vertices[vflag], vrank[m.faces[kept]].astype(np.int32).reshape(-1, 3), vrank[np.clip(m.vertex_start, 0, nv)].astype(np.int64),
               frank[np.clip(m.face_start, 0, nf)].astype(np.int64), None if m.rgb is None else m.rgb[vflag])
    return out, np.nonzero(vflag)[0].astype(np.int32), np.nonzero(kept)[0].astype(np.int32)


def largest(m, comp, k=1):
    """The face mask of each scene's k components with the most faces; between equal counts the lower id."""
    keep_comp = np.zeros(len(comp["faces"]), dtype=bool)
    cs = comp["component_start"]
    for s in range(m.nscene):
        ids = np.arange(cs[s], cs[s + 1])
        order = ids[np.argsort(-comp["faces"][ids].astype(np.int64), kind="stable")]
        keep_comp[order[:k]] = True
    fc = comp["face_component"]
    return (fc >= 0) & keep_comp[np.maximum(fc, 0)] if len(keep_comp) else np.zeros(len(fc), dtype=bool)


def _lists(m):
    """The incidence table padded to (nv, longest list) entries, and each list's length."""
    inc_start, inc = incidence(m)
    nv = len(m.vertices)
    length = np.diff(inc_start.astype(np.int64))
    width = int(length.max()) if nv and len(inc) else 0
    table = np.full((nv, width), -1, dtype=np.int64)
    if width:
        vert = np.repeat(np.arange(nv), length)
        table[vert, np.arange(len(inc)) - inc_start.astype(np.int64)[vert]] = inc
    return table, length


def vertex_normals(m):
    """(float64 (nv, 3) before the rounding, float32 (nv, 3) as the kernel rounds them)."""
    table, length = _lists(m)
    x = m.vertices.astype(np.float64)
    s = np.zeros((len(x), 3), dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(table.shape[1]):
            has = np.nonzero(table[:, j] >= 0)[0]
            ids = m.faces[table[has, j] // 3].astype(np.int64)
            A, B, C = x[ids[:, 0]], x[ids[:, 1]], x[ids[:, 2]]
            ab, ac = B - A, C - A
            s[has, 0] += ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
            s[has, 1] += ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
            s[has, 2] += ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
        norm = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = (norm > 0) & np.isfinite(norm)
        n64 = np.where(ok[:, None], s / np.where(ok, norm, 1.0)[:, None], 0.0)
    return n64, n64.astype(np.float32)


def smooth(m, passes, lam, mu, vertex_flags=None, pin_mask=0):
    """float32 (nv, 3) positions after `passes` umbrella passes with the factors lam, mu, lam, .."""
    table, length = _lists(m)
    x32 = m.vertices.copy()
    pinned = np.zeros(len(x32), dtype=bool) if not pin_mask else (vertex_flags & np.uint8(pin_mask)) != 0
    ent = np.maximum(table, 0)
    fid, corner = ent // 3, ent % 3
    n1 = m.faces[fid, (corner + 1) % 3].astype(np.int64) if table.size else table      # the next corner
    n2 = m.faces[fid, (corner + 2) % 3].astype(np.int64) if table.size else table      # the previous corner
    for p in range(passes):
        f = np.float64(mu if p & 1 else lam)
        x = x32.astype(np.float64)
        S = np.zeros_like(x)
        with np.errstate(all="ignore"):
            for j in range(table.shape[1]):
                has = np.nonzero(table[:, j] >= 0)[0]
                S[has] += x[n1[has, j]]
                S[has] += x[n2[has, j]]
            c = (2 * length).astype(np.float64)
            move = (length > 0) & np.isfinite(S).all(1) & np.isfinite(x).all(1) & ~pinned      # S finite <=> every read coordinate finite
            y = x + f * (S / np.where(length > 0, c, 1.0)[:, None] - x)
            x32 = np.where(move[:, None], y.astype(np.float32), x32)
    return x32


# ------------------------------------------------------------------------------------------------ meshes for the tests
def _quads(quads):
    return [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]


def tetrahedron(offset=(0.0, 0.0, 0.0)):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64) + np.asarray(offset)
    return make(v, [(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)])


def cube(drop_quads=0):
    """The unit cube, vertex id = x + 2 y + 4 z, every quad wound outward and cut along its first diagonal; the last `drop_quads` quads left out."""
    v = [[i & 1, (i >> 1) & 1, i >> 2] for i in range(8)]
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    return make(v, _quads(quads[:6 - drop_quads]))


def permuted(m, perm):
    """The same one-scene mesh with vertex `old` renamed perm[old]."""
    perm = np.asarray(perm)
    v = np.empty_like(m.vertices)
    v[perm] = m.vertices
    rgb = None
    if m.rgb is not None:
        rgb = np.empty_like(m.rgb)
        rgb[perm] = m.rgb
    return Mesh(v, perm[m.faces].astype(np.int32), m.vertex_start, m.face_start, rgb)


def strip(n, seed=0):
    """n triangles in a row over n + 2 vertices, wound alike; slightly bent so that normals and smoothing have something to do."""
    rng = np.random.default_rng(seed)
    i = np.arange(n + 2)
    v = np.stack([i * 0.5, (i & 1).astype(np.float64), 0.1 * rng.standard_normal(n + 2)], axis=1)
    f = [(k, k + 1, k + 2) if k % 2 == 0 else (k + 1, k, k + 2) for k in range(n)]
    return make(v, f)


def fan(n, seed=0):
    """n faces round vertex 0 (an open fan: the rim is a boundary)."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0.0, 1.9 * np.pi, n + 1)
    rim = np.stack([np.cos(a), np.sin(a), 0.05 * rng.standard_normal(n + 1)], axis=1)
    return make(np.concatenate([[[0.0, 0.0, 0.3]], rim]), [(0, k, k + 1) for k in range(1, n + 1)])


def tetrahedra(count):
    ms = [tetrahedron((3.0 * k, 0.0, 0.0)) for k in range(count)]
    v0 = np.cumsum([0] + [4] * count)
    return make(np.concatenate([m.vertices for m in ms]), np.concatenate([m.faces + np.int32(o) for m, o in zip(ms, v0)]))


def quad_grid(n, seed=0, drop=0.0):
    """An n x n quad grid (2 n^2 faces) over a bumpy height field, a share `drop` of its faces removed by seed."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([i / n, j / n, 0.05 * np.sin(7.0 * i / n) * np.cos(5.0 * j / n) + 0.01 * rng.standard_normal(i.shape)], axis=-1).reshape(-1, 3)
    at = lambda jj, ii: jj * (n + 1) + ii
    f = np.array(_quads([(at(jj, ii), at(jj, ii + 1), at(jj + 1, ii + 1), at(jj + 1, ii)) for jj in range(n) for ii in range(n)]))
    return make(v, f[rng.random(len(f)) >= drop])


def with_rgb(m, seed=0):
    m.rgb = np.random.default_rng(100 + seed).random(m.vertices.shape).astype(np.float32)
    return m


def mixed_batch():
    """Two scenes with global ids.  Scene 0: a cube, a detached tetrahedron and an unreferenced vertex.  Scene 1: an open strip with one
    flipped face, a third face on one of its edges, a repeated-id face that joins a lone vertex to a separate triangle, a face that names
    a scene-0 vertex, a face with an id >= nv and one with a negative id (all three invalid)."""
    c, t = cube(), tetrahedron((3.0, 0.0, 0.0))
    s0 = make(np.concatenate([c.vertices, t.vertices, [[9.0, 9.0, 9.0]]]), np.concatenate([c.faces, t.faces + np.int32(8)]))
    st = strip(6, seed=3)
    f = [tuple(int(x) for x in r) for r in st.faces]
    f[3] = (f[3][1], f[3][0], f[3][2])                      # flipped
    f += [(2, 3, 8), (9, 9, 10), (10, 11, 12)]                # three faces on edge 2-3; repeated ids; the piece the repeated face joins
    rng = np.random.default_rng(5)
    s1 = make(np.concatenate([st.vertices, rng.standard_normal((5, 3))]), f)
    m = concat([s0, s1])
    nv = len(m.vertices)
    extra = np.array([[0, 13 + 1, 13 + 2], [13 + 0, 13 + 1, nv + 5], [13 + 4, -1, 13 + 5]], dtype=np.int32)
    m.faces = np.concatenate([m.faces, extra])
    m.face_start = np.array([0, len(s0.faces), len(m.faces)], dtype=np.int64)
    return with_rgb(m, 3)


def scene_of(m, s):
    """Scene s alone, ids un-shifted (an id outside the scene stays outside)."""
    v0, v1, f0, f1 = m.vertex_start[s], m.vertex_start[s + 1], m.face_start[s], m.face_start[s + 1]
    return Mesh(m.vertices[v0:v1], (m.faces[f0:f1].astype(np.int64) - v0).astype(np.int32), np.array([0, v1 - v0]), np.array([0, f1 - f0]),
                None if m.rgb is None else m.rgb[v0:v1])


# ------------------------------------------------------------------------------------------------ the floater volumes of the end-to-end test
BLOB_G, BLOB_HALF, BLOB_BIG_R, BLOB_R = 24, 0.75, 0.45, 0.08
# Towards three corners of the box.  A blob surface lies 0.44 sqrt(3) - 0.08 - 0.45 = 0.232 (3.7 voxels of 0.0625) from the big sphere's
# and 0.75 - 0.44 - 0.08 = 0.23 (3.7 voxels) from the box: the most both can have at once in this box (a sqrt(3) - 0.53 = 0.67 - a at
# a = 0.439), which is why it is not more.
BLOB_CENTRES = ((0.44, 0.44, 0.44), (-0.44, 0.44, -0.44), (0.44, -0.44, -0.44))


def blob_volumes(device="cpu"):
    """(B, U) fp32 (G, G, G) torch volumes in z, y, x order over extract_mesh's default box: the exact signed distance of the big sphere,
    and its minimum with the three small spheres'."""
    import torch
    ax = ((torch.arange(BLOB_G, dtype=torch.float64, device=device) + 0.5) * (2 * BLOB_HALF / BLOB_G) - BLOB_HALF)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    sdf = lambda c, r: (((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2).sqrt() - r).float()
    B = sdf((0.0, 0.0, 0.0), BLOB_BIG_R)
    U = B
    for c in BLOB_CENTRES:
        U = torch.minimum(U, sdf(c, BLOB_R))
    return B, U
