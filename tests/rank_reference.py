"""Serial restatements of the multi-rank arithmetic (csrc/kernels_pcg.hip: k_iface_pack_all / k_iface_unpack, k_p2p_pack /
k_p2p_sum, the owner branches of k_pcg_init / k_update_xr / k_update_d / k_reduce, k_sum_partials2 and the gathered
k_pcg_init_final; csrc/femcy_api.cpp: apply_load's interface sum, the collective femcy_apply_dirichlet_linear), in the dtype the
caller names: float64, or np.longdouble as the reference of tests/rank_shapes.py.  No threads and no torch.distributed: all
ranks run in one Python loop, in rank order, which is the order both exchanges specify.

  iface_sum()        s = 0; for r in sorted(sharing ranks): s += v_r   on every interface DOF, the rest unchanged
  assemble()         the sub-assembled matrix of a rank from its coordinates, every step in the dtype: the float64 twin carries
                     the rounding of an assembly, as a backend's matrix does, and the long-double twin does not
  product()          y_r = K_r x_r with the rank's sub-assembled matrix, then the interface sum
  norm() / absmax()  every shared DOF counted on its owner; RMS over the DOFs of the whole system
  constrain()        rows and columns of the constrained DOFs zeroed, the diagonal = owner[dof]
  dirichlet_linear() rhs -= sum_r K_r s_r, rhs[dofs] = values
  pcg()              the partitioned Jacobi-preconditioned recurrence: M = 1 / interface-summed diagonal, owner-masked r.M.r,
                     d.Ad = sum_r d_r.K_r d_r of the products before their exchange, max|r| over all replicas
  body_weights() / energy_total()
                     m_a = sum N_a |det J| w and the energy of the Green strain from post_reference's Gauss-point pass

No library code runs here."""
import numpy as np

import loads_reference as lr
import post_reference as pr
import thermal_reference as tr

LD = np.longdouble


def gdofs(part):
    """global DOF of every local DOF"""
    return (part.l2g[:, None] * part.dm + np.arange(part.dm)[None, :]).ravel()


def sharing(parts, n_global):
    """bool [n_global, nranks]: DOF held by rank"""
    held = np.zeros((n_global, len(parts)), dtype=bool)
    for p in parts:
        held[gdofs(p), p.rank] = True
    return held


def iface_sum(parts, vecs, dtype):
    nslots = parts[0].niface_global
    acc = np.zeros(nslots, dtype=dtype)                               # s = 0.0
    for p, v in zip(parts, vecs):                                      # ascending rank: s += v_r
        acc[p.iface_global_slot] += np.asarray(v, dtype=dtype)[p.iface_local_dofs]
    out = []
    for p, v in zip(parts, vecs):
        w = np.array(v, dtype=dtype)
        w[p.iface_local_dofs] = acc[p.iface_global_slot]
        out.append(w)
    return out


class Csr:
    """a CSR matrix whose values keep their dtype (scipy has no long-double path): what csr_matvec, constrain and pcg read"""

    def __init__(self, indptr, indices, data, n):
        self.indptr, self.indices, self.data, self.shape = indptr, indices, data, (n, n)

    def tocsr(self):
        return self

    def rows(self):
        return np.repeat(np.arange(self.shape[0]), np.diff(self.indptr))

    def diagonal(self):
        d = np.zeros(self.shape[0], dtype=self.data.dtype)
        on = self.rows() == self.indices
        d[self.indices[on]] = self.data[on]
        return d


def _strain_matrix(dsdx):
    """B(grad N) [ne, npe, dm] -> [ne, s, npe dm], Voigt rows xx, yy, (zz,) xy, (zx, yz): the element classes' strainMtrx"""
    ne, npe, dm = dsdx.shape
    B = np.zeros((ne, 3 if dm == 2 else 6, npe * dm), dtype=dsdx.dtype)
    for i in range(dm):
        B[:, i, i::dm] = dsdx[:, :, i]
    shear = [(0, 1)] if dm == 2 else [(0, 1), (2, 0), (1, 2)]
    for k, (i, j) in enumerate(shear):
        B[:, dm + k, i::dm] = dsdx[:, :, j]
        B[:, dm + k, j::dm] = dsdx[:, :, i]
    return B


def assemble(nodes, el, ELE, C, u, dtype):
    """K = sum_e sum_g B^T C B det J w on the configuration nodes + u, from the coordinates, every step in `dtype`"""
    _, dN, w = lr.element_tables(ELE)
    dN, w, C = dN.astype(dtype), w.astype(dtype), np.asarray(C).astype(dtype)
    dm = nodes.shape[1]
    x = (np.asarray(nodes, dtype=dtype) + np.asarray(u, dtype=dtype).reshape(nodes.shape))[el]
    Ke = 0
    for g in range(len(w)):
        det, inv = tr._det_inv(np.einsum("eai,aj->eij", x, dN[g]))
        B = _strain_matrix(np.einsum("ak,ekj->eaj", dN[g], inv))
        Ke = Ke + np.einsum("epm,pq,eqn,e->emn", B, C, B, det * w[g])
    n = nodes.size
    gd = (el[:, :, None].astype(np.int64) * dm + np.arange(dm)[None, None, :]).reshape(len(el), -1)
    m = gd.shape[1]
    key = (np.repeat(gd, m, axis=1) * n + np.tile(gd, (1, m))).ravel()
    order = np.argsort(key, kind="stable")                              # ascending element inside an entry
    uniq, start = np.unique(key[order], return_index=True)
    data = np.add.reduceat(Ke.ravel()[order], start)
    indptr = np.searchsorted(uniq // n, np.arange(n + 1))
    return Csr(indptr, uniq % n, data, n)


def constrain_csr(K, local_dofs, owner):
    """constrain() on a Csr, in its dtype"""
    mask = np.zeros(K.shape[0], dtype=bool)
    mask[local_dofs] = True
    rows = K.rows()
    data = K.data.copy()
    data[mask[rows] | mask[K.indices]] = 0
    diag = (rows == K.indices) & mask[rows]
    data[diag] = np.asarray(owner)[rows[diag]].astype(data.dtype)
    return Csr(K.indptr, K.indices, data, K.shape[0])


def csr_matvec(K, x, dtype):
    K = K.tocsr()
    prod = K.data.astype(dtype) * np.asarray(x, dtype=dtype)[K.indices]
    y = np.zeros(K.shape[0], dtype=dtype)
    np.add.at(y, np.repeat(np.arange(K.shape[0]), np.diff(K.indptr)), prod)     # row by row, in column order
    return y


def product(parts, Ks, vecs, dtype):
    return iface_sum(parts, [csr_matvec(K, v, dtype) for K, v in zip(Ks, vecs)], dtype)


def norm(parts, vecs, n_global, dtype):
    ss = dtype(0)
    for p, v in zip(parts, vecs):
        w = np.asarray(v, dtype=dtype)[p.owner.astype(bool)]
        ss = ss + (w * w).sum()
    return np.sqrt(ss / dtype(n_global))


def absmax(parts, vecs):
    return max([float(np.abs(np.asarray(v)[p.owner.astype(bool)]).max()) for p, v in zip(parts, vecs) if p.owner.any()] + [0.0])


def constrain(K, local_dofs, owner):
    """the sub-assembled matrix after the 0 / 1 kernel: only the owner contributes the unit diagonal"""
    import scipy.sparse as sp
    from oracle import femcy_oracle as orc
    K = orc._zero_rows_cols_unit_diag(K, np.asarray(local_dofs, dtype=np.int64))
    fix = np.zeros(K.shape[0])
    fix[local_dofs] = 1.0 - np.asarray(owner, dtype=np.float64)[local_dofs]       # 1 - 1 = 0 and 1 - 0 = 1, exactly
    K = (K - sp.diags(fix)).tocsr()
    K.sort_indices()
    return K


def dirichlet_linear(parts, Ks, rhs, dofs, vals, dtype):
    """dofs[r], vals[r]: the prescribed local DOFs rank r holds (possibly none) -> the right-hand sides"""
    s = []
    for p, d, v in zip(parts, dofs, vals):
        sr = np.zeros(p.n_local, dtype=dtype)
        sr[d] = v
        s.append(sr)
    Ks_ = product(parts, Ks, s, dtype)
    out = []
    for b, y, d, v in zip(rhs, Ks_, dofs, vals):
        w = np.asarray(b, dtype=dtype) - y
        w[d] = v
        out.append(w)
    return out


def pcg(parts, Ks, bs, maxit, dtype):
    """-> (x per rank, r0, rmax) after exactly maxit iterations (eps = 0: the stopping rule never fires)"""
    own = [p.owner.astype(dtype) for p in parts]
    M = [dtype(1) / d for d in iface_sum(parts, [K.diagonal() for K in Ks], dtype)]
    r = [np.array(b, dtype=dtype) for b in bs]
    x = [np.zeros_like(b) for b in r]
    d = [m * b for m, b in zip(M, r)]

    def masked(rr):
        s = dtype(0)
        for o, m, v in zip(own, M, rr):
            s = s + (o * (v * m * v)).sum()
        return s

    rMr = masked(r)
    r0 = rmax = max(float(np.abs(v).max()) for v in r)
    for _ in range(maxit):
        Ad = [csr_matvec(K, v, dtype) for K, v in zip(Ks, d)]
        dAd = dtype(0)
        for v, a in zip(d, Ad):                                        # before the exchange: sum_r d_r.K_r d_r
            dAd = dAd + (v * a).sum()
        Ad = iface_sum(parts, Ad, dtype)
        alpha = rMr / dAd
        r = [v - alpha * a for v, a in zip(r, Ad)]
        new = masked(r)
        rmax = max(float(np.abs(v).max()) for v in r)
        beta = new / rMr
        x = [u + alpha * v for u, v in zip(x, d)]
        d = [m * v + beta * w for m, v, w in zip(M, r, d)]
        rMr = new
    return x, r0, rmax


def body_weights(nodes, el, ELE, dtype):
    N = lr.element_tables(ELE)[0].astype(dtype)
    vol = np.abs(pr.gauss_F(nodes, el, ELE, np.zeros(nodes.size), dtype)[1])    # [ne, nGP]
    m = np.zeros(len(nodes), dtype=dtype)
    np.add.at(m, el, np.einsum("eg,ga->ea", vol, N))
    return m


def energy_total(nodes, el, ELE, kind, mat, u, dtype):
    F, vol = pr.gauss_F(nodes, el, ELE, u, dtype)
    return (pr.energy(F, kind, mat.params, mat.C, dtype) * vol).sum()
