"""Reference twin of the wall forces, torque and heat flux (numpy only; test infrastructure, never imported by the product).

Definitions (include/neklab_gpu.h: nlg_forces_*).  A face is (element, face) with face in the preprocessor's numbering
1 = s-, 2 = r+, 3 = s+, 4 = r-, 5 = t-, 6 = t+; its points are those of nekio.face_nodes, in that order.  At face point q of a face normal
to reference direction a on side sigma:  N_q = sigma (J grad r_a)_q w_q, w_q the product of the GLL weights of the other directions.
The gradient is the oracle's element-local `gradm1`; the pressure is the element's Gauss-mesh values carried to the face points by the
tensor Lagrange interpolation GL -> GLL (no average across elements).  Per object, summed over its faces and face points:

    Fp_i = sum p N_i     Fv_i = -nu sum_j (d_j u_i + d_i u_j) N_j     Tp, Tv = sum (x - c) x (.)     Q = sum grad(theta) . N

The face geometry, the pressure extrapolation and the sums are written here on their own; only the metrics and gradm1 are the oracle's.
"""
import numpy as np

FACE_DIR = {1: (1, -1), 2: (0, +1), 3: (1, +1), 4: (0, -1), 5: (2, -1), 6: (2, +1)}   # face -> (reference direction, side)


def nq(dim):
    return 2 * dim + 2 * (1 if dim == 2 else 3) + 1


def face_slice(n, dim, face):
    """index into one element's (n,) * dim array (axes [t,] s, r) that selects the face; the remaining axes ravel to face_nodes' order"""
    a, sg = FACE_DIR[face]
    sl = [slice(None)] * dim
    sl[dim - 1 - a] = 0 if sg < 0 else n - 1
    return tuple(sl)


def face_weights(sem, face):
    """w_q: the GLL weights of the dim - 1 tangential directions, in the order of the face points"""
    w = sem.w1
    return w.copy() if sem.dim == 2 else np.outer(w, w).ravel()


def gl_to_gll(sem):
    """M[i, k] = l_k(z1_i), the Lagrange basis on the Gauss points z2, in product form"""
    z1, z2 = sem.z1, sem.z2
    M = np.ones((len(z1), len(z2)))
    for k in range(len(z2)):
        for l in range(len(z2)):
            if l != k:
                M[:, k] *= (z1 - z2[l]) / (z2[k] - z2[l])
    return M


def pressure_on_mesh1(sem, pr):
    """the element-local extension of the Gauss-mesh pressure to the GLL points (no direct-stiffness average)"""
    M = gl_to_gll(sem)
    p = np.asarray(pr, dtype=np.float64).reshape(sem.shape2)
    for ax in range(1, sem.dim + 1):
        p = np.moveaxis(np.tensordot(M, p, axes=([1], [ax])), 0, ax)
    return p


def geometry(sem, faces, centres=None):
    """faces: [(local element, face)]; centres: one centre per face or None.
    -> N [nf][nfp][dim], G [nf][nfp][dim (j)][dim (i)] = d r_j / d x_i, xc [nf][nfp][dim] = x_q - c"""
    dim, n = sem.dim, sem.n
    N, G, XC = [], [], []
    for q, (e, f) in enumerate(faces):
        a, sg = FACE_DIR[f]
        sl = face_slice(n, dim, f)
        w = face_weights(sem, f)
        jac = sem.jac[e][sl].ravel()
        N.append(np.stack([sg * sem.rst[a][i][e][sl].ravel() * w for i in range(dim)], axis=-1))
        G.append(np.stack([np.stack([sem.rst[j][i][e][sl].ravel() / jac for i in range(dim)], axis=-1) for j in range(dim)], axis=-2))
        c = np.zeros(dim) if centres is None else np.asarray(centres[q], dtype=np.float64)
        XC.append(np.stack([sem.X[i][e][sl].ravel() - c[i] for i in range(dim)], axis=-1))
    return np.array(N), np.array(G), np.array(XC)


def metric_err(sem):
    """Rounding-error bounds of the metrics as whole fields, first order, propagated stage by stage; every stage is (operations on the
    path) x eps x (sum of the absolute values of the summands), two codes that form the same value in different orders differ by at most
    the sum of their bounds, which the constants below already hold:
      a derivative d = sum_m D_m X_m: n products, n - 1 additions, D's entries each a quotient of products of n - 1 node differences
        (2 (2n + 2) for the two codes): c1 = 5n + 5, err(d) = c1 eps sum |D_m| |X_m|;
      a cofactor c = d1 d2 - d3 d4: err(c) = |d1| err(d2) + |d2| err(d1) + |d3| err(d4) + |d4| err(d3) + 2 eps (|d1 d2| + |d3 d4|);
      J = sum_k d_k c_k: err(J) = sum |d_k| err(c_k) + |c_k| err(d_k) + 4 eps sum |d_k c_k|;
      G = c / J: err(G) = err(c) / J + |c| err(J) / J^2 + eps |G|.
    -> cofE[j][i] for J d r_j / d x_i, GE[j][i] for d r_j / d x_i"""
    from oracle.sem import _ap
    dim, n = sem.dim, sem.n
    eps = np.finfo(np.float64).eps
    c1 = 5 * n + 5
    aD = np.abs(sem.D)
    d = [[_ap(sem.D, sem.X[i], sem.axes[j]) for j in range(dim)] for i in range(dim)]            # d x_i / d r_j
    e = [[c1 * eps * _ap(aD, np.abs(sem.X[i]), sem.axes[j]) for j in range(dim)] for i in range(dim)]

    def cof(p1, p2, p3, p4):   # error of d[p1] d[p2] - d[p3] d[p4]
        a, b, c, f = (np.abs(d[p[0]][p[1]]) for p in (p1, p2, p3, p4))
        ea, eb, ec, ef = (e[p[0]][p[1]] for p in (p1, p2, p3, p4))
        return a * eb + b * ea + c * ef + f * ec + 2 * eps * (a * b + c * f)
    if dim == 2:
        cofE = [[e[1][1], e[0][1]], [e[1][0], e[0][0]]]
        jacE = cof((0, 0), (1, 1), (0, 1), (1, 0))
    else:
        cofE = [[cof(((i + 1) % 3, (j + 1) % 3), ((i + 2) % 3, (j + 2) % 3), ((i + 1) % 3, (j + 2) % 3), ((i + 2) % 3, (j + 1) % 3)) for i in range(3)]
                for j in range(3)]
        jacE = sum(np.abs(d[0][k]) * cofE[k][0] + np.abs(sem.rst[k][0]) * e[0][k] + 4 * eps * np.abs(d[0][k] * sem.rst[k][0]) for k in range(3))
    GE = [[cofE[j][i] / sem.jac + np.abs(sem.rst[j][i]) * jacE / sem.jac ** 2 + eps * np.abs(sem.rst[j][i]) / sem.jac for i in range(dim)]
          for j in range(dim)]
    return cofE, GE


def geometry_err(sem, faces):
    """metric_err at the face points: -> NE [nf][nfp][dim], the bound of N_q = sigma c w: err(c) w + (32n + 2) eps |N| (the GLL weights: a
    Legendre recurrence of n - 1 steps of 4 operations, squared, one or two of them, by two codes; the sign and the product), and
    GE [nf][nfp][dim][dim], the bound of the metrics"""
    dim, n = sem.dim, sem.n
    eps = np.finfo(np.float64).eps
    cofE, GEf = metric_err(sem)
    NE, GE = [], []
    for e, f in faces:
        a, sg = FACE_DIR[f]
        sl = face_slice(n, dim, f)
        w = face_weights(sem, f)
        NE.append(np.stack([(cofE[a][i][e][sl].ravel() + (32 * n + 2) * eps * np.abs(sem.rst[a][i][e][sl].ravel())) * w for i in range(dim)], axis=-1))
        GE.append(np.stack([np.stack([GEf[j][i][e][sl].ravel() for i in range(dim)], axis=-1) for j in range(dim)], axis=-2))
    return np.array(NE), np.array(GE)


def fields_of(sem, v):
    """(velocity [dim] on shape1, pressure on shape2, temperature or None) of an oracle vector or a (vel, pr, theta) tuple"""
    if isinstance(v, tuple):
        vel, pr, th = v
    else:
        vel, pr, th = v.v, v.pr, (v.theta[0] if getattr(v, "nscal", 0) else None)
    return [sem.f1(a) for a in vel], sem.f2(pr), (None if th is None else sem.f1(th))


def tractions(sem, faces, v, nu, err=False):
    """per face point: p_q [nf][nfp], the traction p N - nu (grad u + grad u^T) N [nf][nfp][dim], N, and grad(theta) . N (0 without a
    scalar).  err: also the rounding-error bounds (pe, te, qe) of those three, propagated as in metric_err:
      p_q: a tensor contraction over n2^dim Gauss values, dim rows of the GL -> GLL matrix per term (entries as D's, 4 n2 + 4 each):
        err(p) = dim (5 n2 + 5) eps sum |M| |M| |M| |p|;
      a reference derivative of a field: err(ur) = (5n + 5) eps sum |D| |u|;   g_i = sum_j G_ji ur_j:
        err(g_i) = sum_j |G_ji| err(ur_j) + err(G_ji) |ur_j| + (dim + 1) eps sum_j |G_ji ur_j|;
      t_i = p N_i - nu sum_j (g_ij + g_ji) N_j: err(t_i) = err(p) |N_i| + |p| err(N_i) + nu sum_j [(err(g_ij) + err(g_ji)) |N_j| +
        |g_ij + g_ji| err(N_j)] + (2 dim + 4) eps (|p N_i| + nu sum_j (|g_ij| + |g_ji|) |N_j|);  Q = sum_i g_i N_i likewise."""
    dim, n = sem.dim, sem.n
    vel, pr, th = fields_of(sem, v)
    N, _, _ = geometry(sem, faces)
    p1 = pressure_on_mesh1(sem, pr)
    gu = [sem.gradm1(u) for u in vel]                       # gu[i][j] = d_j u_i
    gt = None if th is None else sem.gradm1(th)
    P, T, Q = [], [], []
    for q, (e, f) in enumerate(faces):
        sl = face_slice(n, dim, f)
        p = p1[e][sl].ravel()
        t = np.zeros((p.size, dim))
        for i in range(dim):
            t[:, i] = p * N[q][:, i]
            for j in range(dim):
                t[:, i] -= nu * (gu[i][j][e][sl].ravel() + gu[j][i][e][sl].ravel()) * N[q][:, j]
        P.append(p), T.append(t)
        Q.append(np.zeros(p.size) if gt is None else sum(gt[i][e][sl].ravel() * N[q][:, i] for i in range(dim)))
    out = (np.array(P), np.array(T), N, np.array(Q))
    if not err:
        return out
    from oracle.sem import _ap
    eps = np.finfo(np.float64).eps
    aD, aM = np.abs(sem.D), np.abs(gl_to_gll(sem))
    NE, _ = geometry_err(sem, faces)
    _, GEf = metric_err(sem)
    pe = np.abs(pr)
    for ax in range(1, dim + 1):
        pe = np.moveaxis(np.tensordot(aM, pe, axes=([1], [ax])), 0, ax)
    pe = dim * (5 * sem.n2 + 5) * eps * pe
    G = [[sem.rst[j][i] / sem.jac for i in range(dim)] for j in range(dim)]

    def grad_err(u):   # (error bound, sum of |G ur|) of every component of the gradient
        ur = [_ap(sem.D, u, a) for a in sem.axes]
        ue = [(5 * n + 5) * eps * _ap(aD, np.abs(u), a) for a in sem.axes]
        ab = [sum(np.abs(G[j][i] * ur[j]) for j in range(dim)) for i in range(dim)]
        return [sum(np.abs(G[j][i]) * ue[j] + GEf[j][i] * np.abs(ur[j]) for j in range(dim)) + (dim + 1) * eps * ab[i] for i in range(dim)], ab
    ge = [grad_err(u) for u in vel]
    gte = None if th is None else grad_err(th)
    PE, TE, QE = [], [], []
    for q, (e, f) in enumerate(faces):
        sl = face_slice(n, dim, f)
        aN = np.abs(N[q])
        p, dp = np.abs(P[q]), pe[e][sl].ravel()
        t = np.zeros((p.size, dim))
        for i in range(dim):
            t[:, i] = dp * aN[:, i] + p * NE[q][:, i] + (2 * dim + 4) * eps * p * aN[:, i]
            for j in range(dim):
                gs = np.abs(gu[i][j][e][sl].ravel() + gu[j][i][e][sl].ravel())
                t[:, i] += abs(nu) * ((ge[i][0][j][e][sl].ravel() + ge[j][0][i][e][sl].ravel()) * aN[:, j] + gs * NE[q][:, j]
                                      + (2 * dim + 4) * eps * (ge[i][1][j][e][sl].ravel() + ge[j][1][i][e][sl].ravel()) * aN[:, j])
        PE.append(dp), TE.append(t)
        QE.append(np.zeros(p.size) if gte is None else sum(gte[0][i][e][sl].ravel() * aN[:, i] + np.abs(gt[i][e][sl].ravel()) * NE[q][:, i]
                                                           + (dim + 2) * eps * gte[1][i][e][sl].ravel() * aN[:, i] for i in range(dim)))
    return out + (np.array(PE), np.array(TE), np.array(QE))


def cross(dim, x, f):
    """(x - c) x f per face point: the z component in 2-D, three components in 3-D; -> [..., nt]"""
    if dim == 2:
        return (x[..., 0] * f[..., 1] - x[..., 1] * f[..., 0])[..., None]
    return np.cross(x, f)


def sample(sem, objects, v, nu, centres=None, err=False):
    """objects: list of lists of (local element, face) -> [nobj][NQ] in the order Fp[dim], Fv[dim], Tp[nt], Tv[nt], Q.
    err: also (the rounding-error bound of every sum when its summands carry the bounds of `tractions` and are added in any order, the sum
    of the absolute values of the summands), both of the same shape: bound = sum of the summands' bounds (a torque's cross product with
    x - c: |x| times the force's bound, 4 eps more) + (number of summands) eps (sum of the absolute values)."""
    dim = sem.dim
    eps = np.finfo(np.float64).eps
    out = np.zeros((len(objects), nq(dim)))
    oute, outa = np.zeros_like(out), np.zeros_like(out)
    for o, faces in enumerate(objects):
        if not faces:
            continue
        c = None if centres is None else [centres[o]] * len(faces)
        N, _, XC = geometry(sem, faces, c)
        res = tractions(sem, faces, v, nu, err)
        P, T, Q = res[0], res[1], res[3]
        fp = P[..., None] * N
        fv = T - fp
        parts = [fp, fv, cross(dim, XC, fp), cross(dim, XC, fv), Q[..., None]]
        tot = lambda arrs: np.concatenate([a.reshape(-1, a.shape[-1]).sum(axis=0) for a in arrs])
        out[o] = tot(parts)
        if err:
            PE, TE, QE = res[4], res[5], res[6]
            NE, _ = geometry_err(sem, faces)
            fpe = PE[..., None] * np.abs(N) + np.abs(P)[..., None] * NE + eps * np.abs(fp)
            fve = TE                                   # the viscous part's bound is below the whole traction's
            nt = 1 if dim == 2 else 3
            r = np.abs(XC).sum(axis=-1)[..., None] * np.ones(nt)
            cr = lambda fe, f: r * (fe.max(axis=-1)[..., None] + 4 * eps * np.abs(f).max(axis=-1)[..., None])
            oute[o] = tot([fpe, fve, cr(fpe, fp), cr(fve, fv), QE[..., None]])
            outa[o] = tot([np.abs(fp), np.abs(fv), r * np.abs(fp).max(axis=-1)[..., None], r * np.abs(fv).max(axis=-1)[..., None], np.abs(Q)[..., None]])
            oute[o] += len(faces) * N.shape[1] * eps * outa[o]
    return (out, oute, outa) if err else out


def areas(sem, objects):
    return np.array([np.linalg.norm(geometry(sem, faces)[0], axis=-1).sum() if faces else 0.0 for faces in objects])


def wall_faces(hm):
    """[(local element, face)] of the faces on which every velocity mask is 0 (the walls of a box mesh), ordered by element, then face"""
    from neklab_amd.nekio import face_nodes
    m = np.max(np.stack([np.asarray(a).reshape(hm.E, -1) for a in hm.mask]), axis=0)
    return [(e, f) for e in range(hm.E) for f in range(1, 2 * hm.dim + 1) if np.all(m[e, face_nodes(hm.n, hm.dim, f)] == 0.0)]


# ---------------------------------------------------------------------------------------------------------------------
# the meshes and face lists the CPU and the GPU tests share
# ---------------------------------------------------------------------------------------------------------------------
_cache = {}


def mesh_of(name):
    """A, B: the cases of tests/floquet_ref.py (2-D lx1 = 6 walled box; 3-D lx1 = 8, periodic in x).  N10, N12: a deformed 2 x 1 x 1 box."""
    import floquet_ref as fr
    from neklab_amd.mesh import box_mesh
    from oracle.sem import SEM
    if name in ("A", "B"):
        return fr.case_mesh(name)
    if name not in _cache:
        hm = box_mesh((2, 1, 1), int(name[1:]), lengths=(2.0, 1.0, 1.0), deform=0.05)
        _cache[name] = (hm, SEM(hm))
    return _cache[name]


def case_objects(name, hm):
    """Three objects of (local element, face) that hold every wall face, and on B the interior faces 2 and 4 of element 3 as well, so that
    all 2 dim orientations occur: object 0 = walls normal to y, object 1 = the other walls of the upper half of the elements (no face on
    the first elements), object 2 = the rest.  The corner elements carry faces in two objects."""
    walls = wall_faces(hm)
    obj = [[], [], []]
    for e, f in walls:
        if FACE_DIR[f][0] == 1:
            obj[0].append((e, f))
        elif e >= hm.E - max(1, hm.E // 3):
            obj[1].append((e, f))
        else:
            obj[2].append((e, f))
    if name == "B":
        obj[2] += [(3, 2), (3, 4)]
    return obj


def dns_force_series(sem, cfg, X0, nsteps, objects, centres=None):
    """[nsteps + 1][nobj][NQ]: the twin's forces of the oracle's nonlinear run, stepped exactly as tests/dns_ref.py: run steps it;
    nu = 1 / Re of the run"""
    from oracle.lns import ExptA
    from oracle.vectors import NekDVector
    lane = ExptA(sem, X0.v, cfg)
    lane._reset_state(X0, False)
    lane.nonlinear = True
    cur = NekDVector(sem, X0.nscal, X0.lorder)
    out = []
    for k in range(nsteps + 1):
        if k:
            lane.advance()
        lane._store(cur)
        out.append(sample(sem, objects, cur, 1.0 / cfg.re, centres))
    return np.array(out)
