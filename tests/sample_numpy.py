"""numpy restatement of the area-uniform sample points on a triangle mesh
(csrc/mesh_sample.hip: ucsa_face_sample_counts, ucsa_mesh_surface_samples;
ops.sample_mesh_surface).

Plain loops, one face and one sample at a time.  Every float operation is a
float32 one on numpy scalars in the order the contract names; every hash is
taken in Python integers masked to 32 bits."""
import numpy as np

F = np.float32
M32 = 0xFFFFFFFF
ONE = 1 << 24
INV = F(2.0 ** -24)
R2_A, R2_B = 0xC13FA9A9, 0x91E10DA5


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def face_hashes(seed, f):
    """-> (hc, h1, h2) of face ``f``"""
    h0 = mix((seed & M32) ^ mix(f + 0x9E3779B9))
    return mix(h0 ^ 0x3C6EF372), mix(h0 ^ 0x68BC21EB), mix(h0 ^ 0x02E5BE93)


def _mesh(verts, faces):
    return (np.asarray(verts, F).reshape(-1, 3),
            np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3)))


def face_sample_counts(verts, faces, density, seed=0):
    """-> (area float32 [F], count int32 [F], expect float32 [F])"""
    V, Fc = _mesh(verts, faces)
    nv, nf = V.shape[0], Fc.shape[0]
    with np.errstate(all="ignore"):
        density = F(density)
    if not (density > 0 and np.isfinite(density)):
        raise ValueError("density must be positive and finite in float32")
    area, count, expect = np.zeros(nf, F), np.zeros(nf, np.int32), np.zeros(nf, F)
    with np.errstate(all="ignore"):
        for f in range(nf):
            i0, i1, i2 = (int(x) for x in Fc[f])
            if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= nv:
                continue
            A, B, C = V[i0], V[i1], V[i2]
            e1 = [F(B[k] - A[k]) for k in range(3)]
            e2 = [F(C[k] - A[k]) for k in range(3)]
            cx = F(F(e1[1] * e2[2]) - F(e1[2] * e2[1]))
            cy = F(F(e1[2] * e2[0]) - F(e1[0] * e2[2]))
            cz = F(F(e1[0] * e2[1]) - F(e1[1] * e2[0]))
            a = F(F(0.5) * np.sqrt(F(F(F(cx * cx) + F(cy * cy)) + F(cz * cz))))
            if not (np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(C).all()
                    and np.isfinite(a)):
                continue
            hc = face_hashes(seed, f)[0]
            ex = F(a * density)
            t = np.floor(F(ex + F(F(hc >> 8) * INV)))
            area[f], expect[f] = a, ex
            count[f] = int(t) if t < F(ONE) else ONE
    return area, count, expect


def offsets(count):
    """-> int32 [F+1]: the exclusive prefix sum, taken in Python integers"""
    first, tot = [0], 0
    for c in np.asarray(count).reshape(-1):
        tot += int(c)
        first.append(tot)
    if tot > 2 ** 31 - 1:
        raise ValueError("more than 2^31-1 samples: lower density")
    return np.asarray(first, np.int32)


def find_face(first, nf, s):
    """the bounded upper-bound search of the kernel: the smallest k in [0, nf)
    with first[k+1] > s, then min(k, nf - 1)"""
    lo, hi = 0, nf
    for _ in range(32):
        if lo >= hi:
            break
        mid = (lo + hi) >> 1
        if int(first[mid + 1]) > s:
            hi = mid
        else:
            lo = mid + 1
    return min(lo, nf - 1)


def weights(seed, f, j):
    """-> (c, a, b): the integer weights (of 2^24) of corners 0, 1, 2 of the
    ``j``-th sample of face ``f``"""
    _, h1, h2 = face_hashes(seed, f)
    a = ((j * R2_A + h1) & M32) >> 8
    b = ((j * R2_B + h2) & M32) >> 8
    if a + b > ONE:
        a, b = ONE - a, ONE - b
    return ONE - a - b, a, b


def mesh_surface_samples(verts, faces, first, n_samples, seed=0, normals=None, rgb=None,
                         labels=None):
    """-> dict: points float32 [S,3], face int32 [S], bary float32 [S,3] and, for
    the inputs given, normals float32 [S,3], rgb uint8 [S,3], labels uint8 [S]"""
    V, Fc = _mesh(verts, faces)
    nv, nf, S = V.shape[0], Fc.shape[0], int(n_samples)
    out = {"points": np.zeros((S, 3), F), "face": np.zeros(S, np.int32),
           "bary": np.zeros((S, 3), F)}
    if normals is not None:
        nrm = np.asarray(normals, F).reshape(-1, 3)
        out["normals"] = np.zeros((S, 3), F)
    if rgb is not None:
        col = np.asarray(rgb, np.uint8).reshape(-1, 3)
        out["rgb"] = np.zeros((S, 3), np.uint8)
    if labels is not None:
        lab = np.asarray(labels).astype(np.int64)
        out["labels"] = np.zeros(S, np.uint8)
    with np.errstate(all="ignore"):
        for s in range(S):
            f = find_face(first, nf, s)
            j = (s - int(first[f])) & M32
            c, a, b = weights(seed, f, j)
            w = [F(F(c) * INV), F(F(a) * INV), F(F(b) * INV)]
            out["face"][s] = f
            out["bary"][s] = w
            idx = [int(x) for x in Fc[f]]
            if min(idx) < 0 or max(idx) >= nv:
                continue                                      # zeros (a malformed first only)
            A, B, C = (V[i] for i in idx)
            for k in range(3):
                e1, e2 = F(B[k] - A[k]), F(C[k] - A[k])
                out["points"][s, k] = F(A[k] + F(F(w[1] * e1) + F(w[2] * e2)))
            if normals is not None:
                n = [F(F(F(w[0] * nrm[idx[0], k]) + F(w[1] * nrm[idx[1], k])) +
                       F(w[2] * nrm[idx[2], k])) for k in range(3)]
                ln = F(np.sqrt(F(F(F(n[0] * n[0]) + F(n[1] * n[1])) + F(n[2] * n[2]))))
                for k in range(3):
                    out["normals"][s, k] = F(n[k] / ln) if ln > 0 else F(0)
            if rgb is not None:
                for k in range(3):
                    r = [F(col[i, k]) for i in idx]
                    v = F(F(F(w[0] * r[0]) + F(w[1] * r[1])) + F(w[2] * r[2]))
                    out["rgb"][s, k] = int(np.floor(F(v + F(0.5))))
            if labels is not None:
                corner = 0 if (c >= a and c >= b) else (1 if a >= b else 2)
                out["labels"][s] = lab[idx[corner]]
    return out


def sample_mesh_surface(verts, faces, density, seed=0, normals=None, rgb=None, labels=None,
                        max_samples=1 << 26):
    """The whole of ops.sample_mesh_surface -> dict of numpy arrays (see its
    docstring), and ``expect`` float32 [F]."""
    V, Fc = _mesh(verts, faces)
    if labels is not None:
        l = np.asarray(labels)
        if l.size and (l.min() < 0 or l.max() > 255):
            raise ValueError("labels must be in 0..255")
    area, count, expect = face_sample_counts(V, Fc, density, seed)
    first = offsets(count)
    S = int(first[-1])
    if S > min(int(max_samples), 2 ** 31 - 1):
        raise ValueError(f"{S} samples, more than max_samples: lower density")
    out = mesh_surface_samples(V, Fc, first, S, seed, normals, rgb, labels)
    out.update(area=area, count=count, first=first, n_samples=S, density=float(F(density)),
               expect=expect)
    return out
