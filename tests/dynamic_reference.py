"""numpy restatement of the consistent mass (femcy_mass_*) and of the Newmark recurrence of `solve_dynamic`, in any dtype
(np.longdouble: the reference; np.float64: what its rounding alone is worth), written from the formulas

    m_ab = sum_e sum_q N_a(xi_q) N_b(xi_q) rho |det J_q| w_q,      J_q = X_e^T dN(xi_q)   (undeformed coordinates)
    M a_0 = f(0+);   (K + a0 M) u_{n+1} = f(t_{n+1}) + M (a0 u_n + v_n / (beta dt) + (1 / (2 beta) - 1) a_n)
    a_{n+1} = a0 (u_{n+1} - u_n) - v_n / (beta dt) - (1 / (2 beta) - 1) a_n,   v_{n+1} = v_n + dt ((1 - gamma) a_n + gamma a_{n+1})

with the plug-in's own `mass_rule()` / `shapeFunc` / `dshape_dnat`.  K comes from the oracle (float64, cast).  numpy's linalg
has no long double, hence the small dense L D L^T below; systems stay at <= 300 DOF.  No library code runs here."""
import numpy as np


def _det(J):
    if J.shape[0] == 2:
        return J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0]
    return (J[0, 0] * (J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1]) - J[0, 1] * (J[1, 0] * J[2, 2] - J[1, 2] * J[2, 0])
            + J[0, 2] * (J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0]))


def mass_tables(ELE, dtype):
    pts, w = ELE.mass_rule()
    N = np.array([ELE.shapeFunc(p) for p in pts], dtype=dtype)
    dN = np.array([ELE.dshape_dnat(p) for p in pts], dtype=dtype)
    return N, dN, np.asarray(w, dtype=dtype)


def element_mass(X, tables, rho):
    """[npe, npe] scalars of one element with node coordinates X [npe, dm] (in the tables' dtype)"""
    N, dN, w = tables
    me = np.zeros((X.shape[0], X.shape[0]), dtype=N.dtype)
    for q in range(len(w)):
        me += np.outer(N[q], N[q]) * (rho * (abs(_det(X.T @ dN[q])) * w[q]))
    return me


def mass_matrix(nodes, el, ELE, rho, dtype):
    """dense [nn, nn] scalar mass matrix; the matrix itself is M (x) I_dm"""
    tables = mass_tables(ELE, dtype)
    X = np.asarray(nodes, dtype=dtype)
    M = np.zeros((len(nodes), len(nodes)), dtype=dtype)
    r = dtype(rho)
    for conn in el:
        M[np.ix_(conn, conn)] += element_mass(X[conn], tables, r)
    return M


def mass_volume(nodes, el, ELE, dtype=np.longdouble):
    """the mesh volume by the mass rule (exact where the stiffness rule is not: curved sides)"""
    _, dN, w = mass_tables(ELE, dtype)
    X = np.asarray(nodes, dtype=dtype)
    return sum(abs(_det(X[c].T @ dN[q])) * w[q] for c in el for q in range(len(w)))


def _inv(J):
    d = _det(J)
    if J.shape[0] == 2:
        return np.array([[J[1, 1], -J[0, 1]], [-J[1, 0], J[0, 0]]], dtype=J.dtype) / d
    c = np.empty((3, 3), dtype=J.dtype)
    for i in range(3):
        for j in range(3):
            a, b = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            c[j, i] = (-1) ** (i + j) * (J[a[0], b[0]] * J[a[1], b[1]] - J[a[0], b[1]] * J[a[1], b[0]])
    return c / d


def small_strain_energy(nodes, el, ELE, C, u, dtype):
    """sum over elements and the plug-in's Gauss points of eps^T C eps / 2 |det J| w on the undeformed mesh, eps = sym(F) - I
    the infinitesimal strain of u in the Voigt order of C ([xx, yy, xy] or [xx, yy, zz, xy, zx, yz], engineering shear)"""
    gp = np.asarray(ELE.gaussPoints, dtype=np.float64)
    dN = np.array([ELE.dshape_dnat(p) for p in gp], dtype=dtype)
    w = np.asarray(ELE.gaussWeights, dtype=dtype)
    X, U, C = np.asarray(nodes, dtype=dtype), np.asarray(u, dtype=dtype).reshape(len(nodes), -1), np.asarray(C, dtype=dtype)
    dm = X.shape[1]
    total = dtype(0)
    for conn in el:
        for g in range(len(w)):
            J = X[conn].T @ dN[g]
            # the ABI defines the strain on the deformation gradient it stores: eps = sym(F) - I with F = I + du / dx, so the
            # subtraction costs the digits of 1 / |du / dx| in either format
            F = np.eye(dm, dtype=dtype) + U[conn].T @ (dN[g] @ _inv(J))
            H = (F + F.T) / 2 - np.eye(dm, dtype=dtype)
            if dm == 2:
                ev = np.array([H[0, 0], H[1, 1], 2 * H[0, 1]], dtype=dtype)
            else:
                ev = np.array([H[0, 0], H[1, 1], H[2, 2], 2 * H[0, 1], 2 * H[2, 0], 2 * H[1, 2]], dtype=dtype)
            total += (ev @ C @ ev) / 2 * abs(_det(J)) * w[g]
    return total


def expand(M, dm):
    return np.kron(M, np.eye(dm, dtype=M.dtype))


def ldlt_solve(A, b):
    """x with A x = b for a symmetric positive definite dense A, by L D L^T without pivoting, in A's dtype"""
    n = A.shape[0]
    L = np.array(A, copy=True)
    d = np.zeros(n, dtype=A.dtype)
    for j in range(n):
        d[j] = L[j, j] - (L[j, :j] * L[j, :j] * d[:j]).sum()
        if j + 1 < n:
            L[j + 1:, j] = (L[j + 1:, j] - (L[j + 1:, :j] * (L[j, :j] * d[:j])[None, :]).sum(axis=1)) / d[j]
        L[j, j] = 1
    y = np.array(b, dtype=A.dtype, copy=True)
    for j in range(n):
        y[j] -= (L[j, :j] * y[:j]).sum()
    y /= d
    for j in range(n - 1, -1, -1):
        y[j] -= (L[j + 1:, j] * y[j + 1:]).sum()
    return y


def constrain(A, fixed):
    A = np.array(A, copy=True)
    A[fixed, :] = 0
    A[:, fixed] = 0
    A[fixed, fixed] = 1
    return A


def newmark(M, K, force, fixed, v0, beta, gamma, dt, T, dtype):
    """-> u [steps + 1, n], v, a (same shapes), times.  M, K dense [n, n]; force(t) -> f [n]; fixed = constrained DOFs
    (value 0).  The last step is clipped to T."""
    M, K = np.asarray(M, dtype=dtype), np.asarray(K, dtype=dtype)
    beta, gamma = dtype(beta), dtype(gamma)
    fixed = np.asarray(fixed, dtype=np.int64)
    n = M.shape[0]
    u, v = np.zeros(n, dtype=dtype), np.asarray(v0, dtype=dtype).copy()
    v[fixed] = 0
    f = np.asarray(force(0.0), dtype=dtype).copy()
    f[fixed] = 0
    a = ldlt_solve(constrain(M, fixed), f)
    U, V, A, times = [u.copy()], [v.copy()], [a.copy()], [0.0]
    k, t0 = 0, 0.0
    while t0 < T * (1.0 - 1.0e-12):
        t1 = min((k + 1) * dt, T)
        if T - t1 < 1.0e-12 * T:
            t1 = T
        h = dtype(t1 - t0)
        a0 = 1 / (beta * h * h)
        rhs = np.asarray(force(t1), dtype=dtype) + M @ (a0 * u + v / (beta * h) + (1 / (2 * beta) - 1) * a)
        rhs[fixed] = 0
        un = ldlt_solve(constrain(K + a0 * M, fixed), rhs)
        an = a0 * (un - u) - v / (beta * h) - (1 / (2 * beta) - 1) * a
        v = v + h * ((1 - gamma) * a + gamma * an)
        u, a = un, an
        U.append(u.copy()), V.append(v.copy()), A.append(a.copy()), times.append(t1)
        k, t0 = k + 1, t1
    return np.array(U), np.array(V), np.array(A), np.array(times)
