"""Numpy restatement of the pose-graph optimisation contract (include/rspl.h): the reference
of the pgo tests.  The reference project has no such stage.

poses T_wc as (q xyzw, p); an edge (i, j) measures Z = T_wi^-1 T_wj with weights (w_t, w_r):
    d = R_i^T (p_j - p_i),  e_t = d - t_Z,  e_R = Log(R_Z^T R_i^T R_j)  (through the quaternion, w >= 0)
    F = sum w_t |e_t|^2 + w_r |e_R|^2;  update p <- p + dp, R <- R Exp(dphi)
solve() is the LM rule (include/rspl.h) with a dense Cholesky, or with scipy.sparse's direct solver (sparse=True).
"""
import numpy as np

CONVERGED, MAX_ITERATIONS, STALLED = 0, 1, 2
RESOLVABLE = 1e-12  # a trial whose predicted decrease is at most this share of F ends the call converged


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def qmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def qlog(q):
    q = q / np.linalg.norm(q)
    if q[3] < 0:
        q = -q
    n = np.linalg.norm(q[:3])
    if n < 1e-8:
        return 2.0 * q[:3] / q[3]
    return 2.0 * np.arctan2(n, q[3]) * q[:3] / n


def qexp(phi):
    t = np.linalg.norm(phi)
    if t < 1e-5:
        return np.append((0.5 - t * t / 48.0) * phi, 1.0 - t * t / 8.0)
    return np.append(np.sin(0.5 * t) / t * phi, np.cos(0.5 * t))


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def jr_inv(phi):
    t = np.linalg.norm(phi)
    c = 1.0 / 12.0 if t < 1e-5 else 1.0 / (t * t) - (1.0 + np.cos(t)) / (2.0 * t * np.sin(t))
    S = skew(phi)
    return np.eye(3) + 0.5 * S + c * (S @ S)


def pose_update(q, p, d):
    qn = qmul(q, qexp(d[3:]))
    return qn / np.linalg.norm(qn), p + d[:3]


def edge_residual(qi, pi, qj, pj, qz, pz):
    d = qmat(qi).T @ (pj - pi)
    qe = qmul(qconj(qz), qmul(qconj(qi), qj))
    return np.concatenate([d - pz, qlog(qe)])


def edge_jacobians(qi, pi, qj, pj, qz, pz):
    """e, de/d(delta_i), de/d(delta_j): 6 x 6 each"""
    Ri, Rj = qmat(qi), qmat(qj)
    d = Ri.T @ (pj - pi)
    e = edge_residual(qi, pi, qj, pj, qz, pz)
    A = jr_inv(e[3:])
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Ji[:3, :3] = -Ri.T
    Ji[:3, 3:] = skew(d)
    Ji[3:, 3:] = -A @ Rj.T @ Ri
    Jj[:3, :3] = Ri.T
    Jj[3:, 3:] = A
    return e, Ji, Jj


class Problem:
    def __init__(self, pose_q, pose_p, pose_fixed, edge_i, edge_j, edge_q, edge_p, edge_w):
        self.pose_q = np.ascontiguousarray(pose_q, np.float64).reshape(-1, 4)
        self.pose_p = np.ascontiguousarray(pose_p, np.float64).reshape(-1, 3)
        self.pose_fixed = np.ascontiguousarray(pose_fixed, np.uint8).reshape(-1)
        self.edge_i = np.ascontiguousarray(edge_i, np.int32).reshape(-1)
        self.edge_j = np.ascontiguousarray(edge_j, np.int32).reshape(-1)
        self.edge_q = np.ascontiguousarray(edge_q, np.float64).reshape(-1, 4)
        self.edge_p = np.ascontiguousarray(edge_p, np.float64).reshape(-1, 3)
        self.edge_w = np.ascontiguousarray(edge_w, np.float64).reshape(-1, 2)

    @property
    def n_poses(self):
        return len(self.pose_q)

    @property
    def n_edges(self):
        return len(self.edge_i)

    def free_index(self):
        idx = np.full(self.n_poses, -1, np.int64)
        free = np.flatnonzero(self.pose_fixed == 0)
        idx[free] = np.arange(len(free))
        return idx


def residuals(P, q=None, p=None):
    q = P.pose_q if q is None else q
    p = P.pose_p if p is None else p
    e = np.zeros((P.n_edges, 6))
    for k in range(P.n_edges):
        i, j = P.edge_i[k], P.edge_j[k]
        e[k] = edge_residual(q[i], p[i], q[j], p[j], P.edge_q[k], P.edge_p[k])
    return e


def cost_of(P, e):
    w = np.repeat(P.edge_w, 3, axis=1)
    return float(np.sum(w * e * e))


def cost(P, q=None, p=None):
    return cost_of(P, residuals(P, q, p))


def linearise(P, q=None, p=None, sparse=False):
    """e [E][6], H [6 n_free][6 n_free] (scipy.sparse CSC when sparse), b = -J^T W e"""
    q = P.pose_q if q is None else q
    p = P.pose_p if p is None else p
    fi = P.free_index()
    n = 6 * int((fi >= 0).sum())
    e = np.zeros((P.n_edges, 6))
    b = np.zeros(n)
    rows, cols, vals = [], [], []
    H = None if sparse else np.zeros((n, n))

    def add(a, c, M):
        if sparse:
            r, cc = np.meshgrid(np.arange(6 * a, 6 * a + 6), np.arange(6 * c, 6 * c + 6), indexing="ij")
            rows.append(r.ravel()); cols.append(cc.ravel()); vals.append(M.ravel())
        else:
            H[6 * a:6 * a + 6, 6 * c:6 * c + 6] += M

    for k in range(P.n_edges):
        i, j = P.edge_i[k], P.edge_j[k]
        e[k], Ji, Jj = edge_jacobians(q[i], p[i], q[j], p[j], P.edge_q[k], P.edge_p[k])
        W = np.repeat(P.edge_w[k], 3)
        a, c = fi[i], fi[j]
        if a >= 0:
            add(a, a, Ji.T @ (W[:, None] * Ji))
            b[6 * a:6 * a + 6] -= Ji.T @ (W * e[k])
        if c >= 0:
            add(c, c, Jj.T @ (W[:, None] * Jj))
            b[6 * c:6 * c + 6] -= Jj.T @ (W * e[k])
        if a >= 0 and c >= 0:
            M = Ji.T @ (W[:, None] * Jj)
            add(a, c, M)
            add(c, a, M.T)
    if sparse:
        import scipy.sparse as sp
        if rows:
            H = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsc()
        else:
            H = sp.csc_matrix((n, n))
    return e, H, b


def gradient_norm(P, q, p):
    """|J^T W e| over the free poses at (q, p)"""
    _, _, b = linearise(P, q, p, sparse=P.n_poses > 64)
    return float(np.linalg.norm(b))


def apply_delta(P, q, p, delta):
    fi = P.free_index()
    qn, pn = q.copy(), p.copy()
    for i in np.flatnonzero(fi >= 0):
        qn[i], pn[i] = pose_update(q[i], p[i], delta[6 * fi[i]:6 * fi[i] + 6])
    return qn, pn


def _solve(H, lam, b, sparse):
    """(H + lam I) delta = b, or None where the matrix is not positive definite"""
    n = len(b)
    if sparse:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
        A = (H + lam * sp.identity(n, format="csc")).tocsc()
        try:
            lu = spl.splu(A, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        except RuntimeError:
            return None
        if np.any(lu.U.diagonal() <= 0):
            return None
        return lu.solve(b)
    try:
        L = np.linalg.cholesky(H + lam * np.eye(n))
    except np.linalg.LinAlgError:
        return None
    import scipy.linalg
    return scipy.linalg.cho_solve((L, True), b)


class Result:
    pass


def solve(P, max_iterations=30, step_tol=1e-10, sparse=False):
    R = Result()
    q, p = P.pose_q.copy(), P.pose_p.copy()
    e, H, b = linearise(P, q, p, sparse)
    F = cost_of(P, e)
    R.cost_initial, R.iterations, R.trials, R.status, R.lam = F, 0, 0, CONVERGED, 0.0
    R.n_free = len(b) // 6
    if len(b) > 0 and float(H.diagonal().max()) > 0:  # otherwise nothing to optimise
        lam = 1e-5 * float(H.diagonal().max())
        nu, rejections, R.status = 2.0, 0, MAX_ITERATIONS
        while R.iterations < max_iterations:
            delta = _solve(H, lam, b, sparse)
            R.trials += 1
            ok = False
            if delta is not None:
                if float(delta @ (lam * delta + b)) <= RESOLVABLE * F:  # the cost cannot resolve this step
                    R.status = CONVERGED
                    break
                qn, pn = apply_delta(P, q, p, delta)
                Fn = cost(P, qn, pn)
                with np.errstate(all="ignore"):
                    rho = (F - Fn) / float(delta @ (lam * delta + b))
                ok = bool(rho > 0) and np.isfinite(Fn)
            if ok:
                q, p, F = qn, pn, Fn
                lam *= max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
                nu, rejections = 2.0, 0
                R.iterations += 1
                if np.abs(delta).max() < step_tol:
                    R.status = CONVERGED
                    break
                if R.iterations == max_iterations:
                    break
                e, H, b = linearise(P, q, p, sparse)
            else:
                lam *= nu
                nu *= 2.0
                rejections += 1
                if rejections == 10:
                    R.status = STALLED
                    break
        R.lam = lam
    R.pose_q, R.pose_p, R.cost_final = q, p, F
    return R
