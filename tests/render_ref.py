"""Numpy restatement of the mesh renderer's definition ("Mesh renderer"), brute force over all faces per pixel.

A helper, not a test.  Written from the definition, not from the kernel: it is the yardstick of tests/test_render_gpu.py.  ``dtype``
selects the arithmetic: float64 is the reference, float32 the same formulas at the kernel's precision (how much of an error is
the number format's).  Besides the images it returns two per-pixel margins that say where float32 may legitimately decide otherwise:
``min_w``, the smallest |w_i| over the faces that come within w_i > -0.05 of covering the pixel (an edge passes close to the pixel
centre), and ``gap``, the distance between the two nearest covering depths.
"""
import numpy as np

LIGHT = (0.0, 1.0, 3.0)
BASE = (142.0, 179.0, 247.0)
W_AMBIGUOUS, GAP_AMBIGUOUS = 1e-4, 1e-5


def default_transform(scale=1.0):
    return np.array([[-1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 2.0 * scale]])


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _normalize(x, eps):
    return x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), eps)


def render_ref(verts, faces, S, scale=1.0, transform=None, focal=None, dtype=np.float64, chunk_elems=1 << 21, detail=False):
    """verts (T, V, 3), faces (F, 3) -> dict(rgb (T,3,S,S), alpha (T,1,S,S), pix_to_face (T,S,S) int32, min_w (T,S,S), gap (T,S,S)).
    ``detail=True`` adds ``wmin`` and ``pz`` (T, F, S*S): per face and pixel the smallest w_i (-inf for a skipped face) and the depth."""
    dt = np.dtype(dtype).type
    verts = np.asarray(verts).astype(dtype)
    faces = np.asarray(faces).astype(np.int64)
    T, V, F, P = verts.shape[0], verts.shape[1], faces.shape[0], S * S
    M = (default_transform(scale) if transform is None else np.asarray(transform)).astype(dtype).reshape(3, 4)
    R, Tv = M[:, :3], M[:, 3]
    f = dt(12.0 if focal is None else focal)
    centre = -(Tv @ R.T)
    coord = dt(1) - (2 * np.arange(S) + 1).astype(dtype) / dt(S)      # pixel centres; +x is left, +y is up
    PX, PY = np.tile(coord, S), np.repeat(coord, S)                    # pixel p = row * S + column
    light, base = np.array(LIGHT, dtype=dtype), np.array(BASE, dtype=dtype) / dt(255)
    eps6, eps8 = dt(1e-6), dt(1e-8)
    out = dict(rgb=np.empty((T, 3, P), dtype), alpha=np.empty((T, 1, P), dtype), pix_to_face=np.empty((T, P), np.int32),
               min_w=np.empty((T, P), dtype), gap=np.empty((T, P), dtype))
    if detail:
        out["wmin"], out["pz"] = np.empty((T, F, P), dtype), np.empty((T, F, P), dtype)
    step = max(1, chunk_elems // max(F, 1))
    for t in range(T):
        vw = verts[t]
        with np.errstate(all="ignore"):
            view = vw @ R + Tv
            Z = view[:, 2]
            xn, yn = f * view[:, 0] / Z, f * view[:, 1] / Z
        i0, i1, i2 = faces[:, 0], faces[:, 1], faces[:, 2]
        z0, z1, z2 = Z[i0][:, None], Z[i1][:, None], Z[i2][:, None]
        with np.errstate(all="ignore"):
            area = _edge(xn[i2], yn[i2], xn[i0], yn[i0], xn[i1], yn[i1])
        valid = (np.abs(area) > eps8) & (Z[i0] > eps6) & (Z[i1] > eps6) & (Z[i2] > eps6)
        # vertex normals: sum of the face cross products over the faces that hold the vertex
        fn = np.cross(vw[i1] - vw[i0], vw[i2] - vw[i0])
        vn = np.zeros((V, 3), dtype)
        for c in range(3):
            np.add.at(vn, faces[:, c], fn)
        vn = _normalize(vn, eps6)
        for p0 in range(0, P, step):
            px, py = PX[None, p0:p0 + step], PY[None, p0:p0 + step]
            n = px.shape[1]
            with np.errstate(all="ignore"):
                a = area[:, None]
                w0 = _edge(px, py, xn[i1][:, None], yn[i1][:, None], xn[i2][:, None], yn[i2][:, None]) / a
                w1 = _edge(px, py, xn[i2][:, None], yn[i2][:, None], xn[i0][:, None], yn[i0][:, None]) / a
                w2 = _edge(px, py, xn[i0][:, None], yn[i0][:, None], xn[i1][:, None], yn[i1][:, None]) / a
                t0, t1, t2 = w0 * z1 * z2, z0 * w1 * z2, z0 * z1 * w2
                den = np.maximum(t0 + t1 + t2, eps8)
                b0, b1, b2 = t0 / den, t1 / den, t2 / den
                pz = b0 * z0 + b1 * z1 + b2 * z2
                cover = valid[:, None] & (w0 > 0) & (w1 > 0) & (w2 > 0) & ~(pz < 0)
                near = valid[:, None] & (w0 > -0.05) & (w1 > -0.05) & (w2 > -0.05)
                wabs = np.minimum(np.minimum(np.abs(w0), np.abs(w1)), np.abs(w2))
            pzc = np.where(cover, pz, np.inf)
            win = np.argmin(pzc, axis=0)                  # the first minimum: equal depths go to the lower face index
            covered = cover.any(axis=0)
            cols = np.arange(n)
            out["min_w"][t, p0:p0 + n] = np.where(near, wabs, np.inf).min(axis=0)
            if F > 1:
                two = np.partition(pzc, 1, axis=0)[:2]
                with np.errstate(all="ignore"):
                    gap = two[1] - two[0]
                out["gap"][t, p0:p0 + n] = np.where(np.isfinite(two[1]), gap, np.inf)
            else:
                out["gap"][t, p0:p0 + n] = np.inf
            if detail:
                out["wmin"][t, :, p0:p0 + n] = np.where(valid[:, None], np.minimum(np.minimum(w0, w1), w2), -np.inf)
                out["pz"][t, :, p0:p0 + n] = pz
            # shading of the winner
            fw = faces[win]
            bw = np.stack([b0[win, cols], b1[win, cols], b2[win, cols]], axis=1)      # (n, 3)
            with np.errstate(all="ignore"):
                Pw = (bw[:, :, None] * vw[fw]).sum(axis=1)
                Nw = _normalize((bw[:, :, None] * vn[fw]).sum(axis=1), eps6)
                d = _normalize(light[None] - Pw, eps6)
                c = (Nw * d).sum(-1)
                v = _normalize(centre[None] - Pw, eps6)
                r = -d + dt(2) * c[:, None] * Nw
                al = np.where(c > 0, np.maximum((v * r).sum(-1), dt(0)), dt(0))
                colour = (dt(0.5) + dt(0.3) * np.maximum(c, dt(0)))[:, None] * base[None] + (dt(0.2) * dt(0.6) * al ** 10)[:, None]
            out["rgb"][t, :, p0:p0 + n] = np.where(covered[None], dt(255) * colour.T, dt(255))
            out["alpha"][t, 0, p0:p0 + n] = covered.astype(dtype)
            out["pix_to_face"][t, p0:p0 + n] = np.where(covered, win, -1)
    for k, shape in (("rgb", (T, 3, S, S)), ("alpha", (T, 1, S, S)), ("pix_to_face", (T, S, S)), ("min_w", (T, S, S)), ("gap", (T, S, S))):
        out[k] = out[k].reshape(shape)
    return out


def ambiguous(ref):
    """Pixels where float32 may legitimately pick another face than float64: an edge within 1e-4 (in barycentric units) of the pixel
    centre, or two covering depths within 1e-5."""
    return (ref["min_w"] < W_AMBIGUOUS) | (ref["gap"] < GAP_AMBIGUOUS)


# ---------------------------------------------------------------------------------------------- meshes of the tests
def uv_sphere(n_lon=24, n_lat=16, radius=0.12, x_scale=0.8):
    """(n_lat + 1) rows of n_lon vertices, poles on the y axis (each pole is a row of coincident vertices), two triangles per quad:
    2 * n_lon * n_lat faces."""
    lat = np.pi * np.arange(n_lat + 1) / n_lat
    lon = 2.0 * np.pi * np.arange(n_lon) / n_lon
    la, lo = np.meshgrid(lat, lon, indexing="ij")
    v = np.stack([x_scale * radius * np.sin(la) * np.cos(lo), radius * np.cos(la), radius * np.sin(la) * np.sin(lo)], -1).reshape(-1, 3)
    faces = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
            c, d = a + n_lon, b + n_lon
            faces += [(a, b, c), (b, d, c)]      # outward normals
    return v, np.array(faces, dtype=np.int32)


def jittered_sphere(T=3, seed=11, sigma=0.003):
    """The test mesh: T frames of the 768-face sphere, every vertex moved by N(0, sigma) per frame.  float32 vertices (what the
    device gets), faces int32."""
    v, faces = uv_sphere()
    g = np.random.default_rng(seed)
    verts = v[None] + sigma * g.standard_normal((T,) + v.shape)
    return verts.astype(np.float32), faces
