"""Tetrahedral test meshes: a conforming Kuhn (Freudenthal) split of an N^3 cube and writers for MFEM mesh v1.0 and Gmsh 2.2.

Every cell of the unit-cube grid is cut into 6 tetrahedra along its main diagonal (vertex 0 -> 7), the same diagonal in every cell, so the
faces match across cells.  Boundary triangles carry the reference's face ids (1 z-min, 2 x-min, 3 y-min, 4 z-max, 5 x-max, 6 y-max).
"""
import itertools
import os

import numpy as np

REFDATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refdata")


def refdata_grains():
    return np.loadtxt(os.path.join(REFDATA, "grains.txt")).astype(int).ravel()


def kuhn_cube(N, perturb=0.0, shuffle=False, seed=0, grains="refdata"):
    """X (NV, 3), tets (E, 4) positively oriented, attr (E,), tris (B, 3), tri_attr (B,).
    grains: "refdata" (cell (i, j, k) takes the grain of the 5^3 cell it falls in, refdata/grains.txt, x fastest), "one", or an array (N^3,).
    perturb: random displacement of interior vertices, as a fraction of the cell size.  shuffle: elements and vertices permuted."""
    rng = np.random.default_rng(seed)
    n1 = N + 1
    g = np.arange(n1)
    X = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).transpose(2, 1, 0, 3).reshape(-1, 3).astype(float) / N   # x fastest
    vid = lambda i, j, k: i + n1 * (j + n1 * k)  # noqa: E731
    if grains == "refdata":
        g5 = refdata_grains()
        cell_grain = lambda i, j, k: g5[(i * 5 // N) + 5 * ((j * 5 // N) + 5 * (k * 5 // N))]  # noqa: E731
    elif grains == "one":
        cell_grain = lambda i, j, k: 1  # noqa: E731
    else:
        ga = np.asarray(grains).ravel()
        cell_grain = lambda i, j, k: ga[i + N * (j + N * k)]  # noqa: E731
    tets, attr = [], []
    for k in range(N):
        for j in range(N):
            for i in range(N):
                for perm in itertools.permutations(range(3)):
                    path = [np.zeros(3, int)]
                    for ax in perm:
                        nxt = path[-1].copy(); nxt[ax] = 1; path.append(nxt)
                    tets.append([vid(i + o[0], j + o[1], k + o[2]) for o in path])
                    attr.append(cell_grain(i, j, k))
    tets = np.array(tets, dtype=np.int64); attr = np.array(attr, dtype=np.int64)
    if perturb > 0:
        inner = np.all((X > 1e-12) & (X < 1 - 1e-12), axis=1)
        X[inner] += perturb / N * rng.uniform(-1, 1, size=(inner.sum(), 3))
    # orientation
    a = X[tets[:, 1]] - X[tets[:, 0]]; b = X[tets[:, 2]] - X[tets[:, 0]]; c = X[tets[:, 3]] - X[tets[:, 0]]
    neg = np.einsum("ij,ij->i", a, np.cross(b, c)) < 0
    tets[neg, 2], tets[neg, 3] = tets[neg, 3].copy(), tets[neg, 2].copy()
    # boundary triangles: faces used once
    faces = {}
    for t in tets:
        for f in ((t[0], t[1], t[2]), (t[0], t[1], t[3]), (t[0], t[2], t[3]), (t[1], t[2], t[3])):
            key = tuple(sorted(f)); faces[key] = faces.get(key, 0) + 1
    tris, tri_attr = [], []
    for f, cnt in faces.items():
        if cnt != 1:
            continue
        P = X[list(f)]
        for d, lo_id, hi_id in ((2, 1, 4), (0, 2, 5), (1, 3, 6)):
            if np.all(np.abs(P[:, d]) < 1e-12):
                tris.append(f); tri_attr.append(lo_id); break
            if np.all(np.abs(P[:, d] - 1) < 1e-12):
                tris.append(f); tri_attr.append(hi_id); break
    tris = np.array(tris, dtype=np.int64); tri_attr = np.array(tri_attr, dtype=np.int64)
    if shuffle:
        pe = rng.permutation(len(tets)); tets, attr = tets[pe], attr[pe]
        pv = rng.permutation(len(X)); inv = np.empty_like(pv); inv[pv] = np.arange(len(pv))
        X = X[pv]; tets = inv[tets]; tris = inv[tris]
    return {"X": X, "tets": tets, "attr": attr, "tris": tris, "tri_attr": tri_attr}


def write_mfem(path, m, nodes_gf=False):
    with open(path, "w") as f:
        f.write("MFEM mesh v1.0\n\ndimension\n3\n\nelements\n%d\n" % len(m["tets"]))
        for a, t in zip(m["attr"], m["tets"]):
            f.write("%d 4 %d %d %d %d\n" % (a, *t))
        f.write("\nboundary\n%d\n" % len(m["tris"]))
        for a, t in zip(m["tri_attr"], m["tris"]):
            f.write("%d 2 %d %d %d\n" % (a, *t))
        f.write("\nvertices\n%d\n" % len(m["X"]))
        if nodes_gf:
            f.write("\nnodes\nFiniteElementSpace\nFiniteElementCollection: H1_3D_P1\nVDim: 3\nOrdering: 1\n\n")
        else:
            f.write("3\n")
        for x in m["X"]:
            f.write("%.17g %.17g %.17g\n" % tuple(x))
    return path


def write_gmsh(path, m):
    """Gmsh 2.2 ASCII; node ids are 1-based and offset (readers must map them), triangles before tetrahedra, as Neper writes them."""
    off = 100
    with open(path, "w") as f:
        f.write("$MeshFormat\n2.2 0 8\n$EndMeshFormat\n$Nodes\n%d\n" % len(m["X"]))
        for i, x in enumerate(m["X"]):
            f.write("%d %.17g %.17g %.17g\n" % (i + off, *x))
        f.write("$EndNodes\n$Elements\n%d\n" % (len(m["tris"]) + len(m["tets"])))
        k = 1
        for a, t in zip(m["tri_attr"], m["tris"]):
            f.write("%d 2 2 %d %d %d %d %d\n" % (k, a, a, *(t + off))); k += 1
        for a, t in zip(m["attr"], m["tets"]):
            f.write("%d 4 2 %d %d %d %d %d %d\n" % (k, a, a, *(t + off))); k += 1
        f.write("$EndElements\n")
    return path


def tet_volumes(X, tets):
    a = X[tets[:, 1]] - X[tets[:, 0]]; b = X[tets[:, 2]] - X[tets[:, 0]]; c = X[tets[:, 3]] - X[tets[:, 0]]
    return np.einsum("ij,ij->i", a, np.cross(b, c)) / 6.0


def ref_tables_numpy(p):
    """Independent construction of the tetrahedron tables: G (n,3,Q) flat, W (Q), N (n,Q) flat, from the barycentric rule."""
    if p == 1:
        pts = [(0.25,) * 4] + [tuple(0.5 if i == k else 1 / 6 for i in range(4)) for k in range(4)]
        w = [-2 / 15] + [3 / 40] * 4
    else:
        a = 0.045503704125649649492; b = 0.5 - a
        pts, w = [], []
        for i, j in itertools.combinations(range(4), 2):
            pts.append(tuple(a if m in (i, j) else b for m in range(4))); w.append(7.0910034628469110730e-3)
        for aa, ww in ((0.092735250310891226402, 0.012248840519393658257), (0.31088591926330060980, 0.018781320953002641800)):
            for k in range(4):
                pts.append(tuple(1 - 3 * aa if m == k else aa for m in range(4))); w.append(ww)
    dL = np.array([[-1, -1, -1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    edges = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    n = 4 if p == 1 else 10
    Q = len(pts)
    G = np.zeros((Q, 3, n)); N = np.zeros((Q, n))
    for q, L in enumerate(pts):
        for v in range(4):
            if p == 1:
                N[q, v] = L[v]; G[q, :, v] = dL[v]
            else:
                N[q, v] = L[v] * (2 * L[v] - 1); G[q, :, v] = (4 * L[v] - 1) * dL[v]
        if p == 2:
            for e, (i, j) in enumerate(edges):
                N[q, 4 + e] = 4 * L[i] * L[j]; G[q, :, 4 + e] = 4 * (L[j] * dL[i] + L[i] * dL[j])
    return G.ravel(), np.array(w), N.ravel()
