"""A plain-numpy, extended-precision statement of one step of the least-squares refit (rh_refit_lsq / orc_refit_lsq),
written from the geometry: the signed distance of a point to a sphere, a cylinder, a cone as a function of the step x in
the documented parametrisation, its Jacobian by central differences in np.longdouble (no analytic row anywhere in this
file), the damped normal equations summed and solved in np.longdouble.  The plane is total least squares: centroid and
smallest eigenvector of the scatter about the centroid.

Shapes are (name, outwards, v) with v in the rh_shape field order, as synth.jittered_candidates returns them:
    plane     v = point[3] normal[3]
    sphere    v = centre[3] R
    cylinder  v = axis[3] centre[3] R
    cone      v = apex[3] axis[3] opang

The step x:
    sphere    centre += x[0:3], R += x[3]
    cylinder  centre += x0 e1 + x1 e2, axis = unit(axis + x2 e1 + x3 e2), R += x4
    cone      apex += x[0:3], axis = unit(axis + x3 e1 + x4 e2), opang += 2 x5
with e1, e2 the frame of the current axis: t = the coordinate direction of the axis' smallest component (the first of
equal ones), e1 = unit(axis x t), e2 = unit(axis x e1).

Accuracy of the differences.  A step of 1e-6 of the scene scale with the 2-point difference leaves a truncation error
of ~1e-12 relative and, with r evaluated to ~1e-17 (coordinates of size <= 100, u_l = 2^-64) and divided by h = 1e-4,
a rounding error of 1e-13: both above what the one-step bound allows the reference where few points are selected
(n_sel u = 1e-15 at 8 points).  So the differences are taken with the 7-point central stencil (h, 2h, 3h; weights 3/4,
-3/20, 1/60; truncation (36/5040) h^6 r^(7)) at the larger step h = STEP_REL * scale, STEP_REL = 1e-4: 1e-2 for the
length columns (scale = the scene's 100), 1e-4 for the angle columns (scale 1).  r is smooth in x on the length scale rho
= the distance of the point from the centre / axis, >= 0.9 here (a cone's points nearest the apex), 3..15 otherwise:
truncation (1e-2 / 3)^6 * 36 / 5040 ~ 1e-17 (1e-14 for the few points at rho ~ 1), rounding 1e-17 / 1e-2 ~ 1e-15 per
entry and random from point to point.  Doubling STEP_REL moves the step x by less than 1 % of the one-step bound in
every case of tests/test_lsq_host.py."""
import numpy as np

LD = np.longdouble
KIND = {"plane": 0, "sphere": 1, "cylinder": 2, "cone": 3}
NPAR = {"plane": 6, "sphere": 4, "cylinder": 7, "cone": 7}     # leading fields of v that describe the shape
NCOL = {"sphere": 4, "cylinder": 5, "cone": 6}
SCENE = 100.0          # synth.BOX: the scale of every coordinate
STEP_REL = 1e-4
DAMP = LD(1e-12)
_STENCIL = ((1, LD(3) / LD(4)), (2, -LD(3) / LD(20)), (3, LD(1) / LD(60)))


def _ld(a):
    return np.asarray(a, dtype=LD)


def _unit(a):
    return a / np.sqrt((a * a).sum())


def frame(axis):
    """e1, e2 perpendicular to the axis; the fixed direction is the coordinate axis of its smallest component"""
    a = _ld(axis)
    k = 0
    for i in (1, 2):
        if abs(a[i]) < abs(a[k]):
            k = i
    t = np.zeros(3, dtype=LD)
    t[k] = 1
    e1 = _unit(np.cross(a, t))
    e2 = _unit(np.cross(a, e1))
    return e1, e2


def moved(name, v, x, fr=None):
    """the shape v after the step x (np.longdouble); fr = the frame of the axis of v"""
    v, x = _ld(v)[:NPAR[name]].copy(), _ld(x)
    if name == "sphere":
        v[0:4] += x[0:4]
        return v
    if name == "cylinder":
        e1, e2 = fr if fr is not None else frame(v[0:3])
        v[3:6] += x[0] * e1 + x[1] * e2
        v[0:3] = _unit(v[0:3] + x[2] * e1 + x[3] * e2)
        v[6] += x[4]
        return v
    e1, e2 = fr if fr is not None else frame(v[3:6])
    v[0:3] += x[0:3]
    v[3:6] = _unit(v[3:6] + x[3] * e1 + x[4] * e2)
    v[6] += 2 * x[5]
    return v


def distance(name, v, P):
    """signed geometric distance of the points P (m, 3) to the shape v, np.longdouble"""
    v, P = _ld(v), _ld(P)
    if name == "plane":
        return (P - v[0:3]) @ _unit(v[3:6])
    if name == "sphere":
        d = P - v[0:3]
        return np.sqrt((d * d).sum(axis=1)) - v[3]
    if name == "cylinder":
        a, t = v[0:3], P - v[3:6]
    else:
        a, t = v[3:6], P - v[0:3]
    h = t @ a
    q = t - h[:, None] * a
    rho = np.sqrt((q * q).sum(axis=1))
    if name == "cylinder":
        return rho - v[6]
    phi = v[6] / 2
    return rho * np.cos(phi) - h * np.sin(phi)


def steps(name):
    hl, ha = LD(STEP_REL * SCENE), LD(STEP_REL)
    return {"sphere": [hl] * 4, "cylinder": [hl, hl, ha, ha, hl], "cone": [hl, hl, hl, ha, ha, ha]}[name]


def residual_and_jacobian(name, v, P):
    """r (m,) at x = 0 and J (m, ncol) = dr/dx at x = 0 by central differences of distance(moved(v, x))"""
    m = NCOL[name]
    axis = None if name == "sphere" else (_ld(v)[0:3] if name == "cylinder" else _ld(v)[3:6])
    fr = None if axis is None else frame(axis)
    r = distance(name, moved(name, v, np.zeros(m), fr), P)
    J = np.zeros((P.shape[0], m), dtype=LD)
    for j, h in enumerate(steps(name)):
        for k, w in _STENCIL:
            x = np.zeros(m, dtype=LD)
            x[j] = k * h
            rp = distance(name, moved(name, v, x, fr), P)
            rm = distance(name, moved(name, v, -x, fr), P)
            J[:, j] += w * (rp - rm) / h
    return r, J


def _fsum_ld(a):
    """sum of a longdouble vector: pairwise in longdouble (numpy), the error is ~log2(m) 2^-64 of the sum of magnitudes"""
    return np.add.reduce(a, dtype=LD)


def normal_equations(r, J):
    m = J.shape[1]
    A = np.zeros((m, m), dtype=LD)
    b = np.zeros(m, dtype=LD)
    for i in range(m):
        b[i] = _fsum_ld(J[:, i] * r)
        for j in range(i, m):
            A[i, j] = A[j, i] = _fsum_ld(J[:, i] * J[:, j])
    return A, b, _fsum_ld(r * r)


def solve_ld(A, b):
    """Gaussian elimination with partial pivoting in np.longdouble"""
    m = len(b)
    M = np.concatenate([_ld(A).copy(), _ld(b).reshape(m, 1)], axis=1)
    for k in range(m):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        for i in range(k + 1, m):
            M[i, k:] -= (M[i, k] / M[k, k]) * M[k, k:]
    x = np.zeros(m, dtype=LD)
    for i in range(m - 1, -1, -1):
        x[i] = (M[i, m] - M[i, i + 1:m] @ x[i + 1:m]) / M[i, i]
    return x


def select(shape, xyz, nrm, enabled, params):
    """the enabled points compatible with the shape at 3 eps[kind] and cos_alpha[kind] -> bool (n,)"""
    from test_oracle_numpy_twin import compat_cone, compat_cylinder, compat_plane, compat_sphere
    name, outw, v = shape
    v = np.asarray(v, dtype=np.float64)
    k = KIND[name]
    eps, cosa = 3.0 * params.eps[k], params.cos_alpha[k]
    with np.errstate(all="ignore"):
        if name == "plane":
            m = compat_plane(v[0:3], v[3:6], xyz, nrm, eps, cosa)
        elif name == "sphere":
            m = compat_sphere(v[0:3], v[3], outw, xyz, nrm, eps, cosa)
        elif name == "cylinder":
            m = compat_cylinder(v[0:3], v[3:6], v[6], outw, xyz, nrm, eps, cosa)
        else:
            m = compat_cone(v[0:3], v[3:6], v[6], outw, xyz, nrm, eps, cosa)
    return m if enabled is None else m & np.asarray(enabled, dtype=bool)


def plane_step(v, P):
    """total least squares: -> new v, rms = sqrt(lambda_min / N), x = new v - v, kappa = lambda_max / (lambda_mid -
    lambda_min) (what a relative perturbation of the scatter is multiplied by on its way into the normal), and the
    in-plane spread sigma^2 = lambda_max / N"""
    v, P = _ld(v)[:6], _ld(P)
    N = P.shape[0]
    cen = np.array([_fsum_ld(P[:, i]) for i in range(3)], dtype=LD) / N
    d = P - cen
    S = np.zeros((3, 3), dtype=LD)
    for i in range(3):
        for j in range(i, 3):
            S[i, j] = S[j, i] = _fsum_ld(d[:, i] * d[:, j])
    w, V = np.linalg.eigh(S.astype(np.float64))
    n = V[:, 0]
    # one step of inverse iteration in longdouble takes the eigenvector from float64's to the scatter's own accuracy
    n = _ld(n)
    lam = n @ S @ n
    B = S - lam * np.eye(3, dtype=LD)
    k = int(np.argmax(np.abs(n)))          # fix the largest component, solve the other two rows
    idx = [i for i in range(3) if i != k]
    rhs = -B[np.ix_(idx, [k])][:, 0] * n[k]
    sol = solve_ld(B[np.ix_(idx, idx)], rhs)
    n2 = n.copy()
    n2[idx] = sol
    n = _unit(n2)
    lam = _fsum_ld((d @ n) ** 2)           # = n' S n without its cancellation
    if n @ v[3:6] < 0:
        n = -n
    new = np.concatenate([cen, n])
    rms = np.sqrt(max(lam, LD(0)) / N)
    kappa = float(w[2] / (w[1] - w[0]))
    return new, rms, new - v, kappa, float(w[2] / N)


class Step:
    pass


def one_step(shape, xyz, nrm, enabled, params):
    """-> Step with .v (the new shape's fields, np.longdouble), .n_sel, .rms (of the input shape over the selection; the
    plane: of the fitted plane), .x (the step), .kappa (condition number of D A D, D = diag(A)^(-1/2); the plane: see
    plane_step), .sel (bool mask)"""
    name, outw, v = shape
    st = Step()
    st.sel = select(shape, xyz, nrm, enabled, params)
    st.n_sel = int(st.sel.sum())
    P = xyz[st.sel]
    if name == "plane":
        st.v, st.rms, st.x, st.kappa, st.sigma2 = plane_step(v, P)
        return st
    r, J = residual_and_jacobian(name, v, P)
    A, b, rr = normal_equations(r, J)
    d = 1 / np.sqrt(np.diag(A))
    st.kappa = float(np.linalg.cond((A * d[:, None] * d[None, :]).astype(np.float64)))
    Ad = A + DAMP * np.trace(A) * np.eye(len(b), dtype=LD)
    st.x = solve_ld(Ad, -b)
    st.v = moved(name, v, st.x)
    st.rms = np.sqrt(rr / st.n_sel)
    return st


def gradient(shape, P):
    """-> (|J'r|, |J| |r|) of the shape over the points P (Frobenius norm of J): zero gradient = a least-squares fit"""
    name, outw, v = shape
    r, J = residual_and_jacobian(name, v, P)
    g = np.array([_fsum_ld(J[:, i] * r) for i in range(J.shape[1])], dtype=LD)
    return float(np.sqrt((g * g).sum())), float(np.sqrt(_fsum_ld((J * J).ravel())) * np.sqrt(_fsum_ld(r * r)))


def one_step_bound(c, st, v_in, name):
    """c n_sel u kappa |x|_inf + 8 u |p|_inf with u = 2^-53"""
    u = 2.0 ** -53
    xinf = float(np.abs(st.x).max())
    pinf = float(np.abs(np.asarray(v_in, dtype=np.float64)[:NPAR[name]]).max())
    return c * st.n_sel * u * st.kappa * xinf + 8 * u * pinf
