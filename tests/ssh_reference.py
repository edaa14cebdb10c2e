"""Dense, plain-numpy restatement of the bond-phonon (SSH) model for small systems — test infrastructure.

The generalisation of tests/golden/make_golden.py's raw_table / checkerboard_order / dense_cb / dense_M / gen_ssh to any
lattice (orbitals, L1 x L2 x L3 cells, any list of bond definitions, a phonon flag per definition).  It imports neither the
product's lattice module nor the oracle: the tables come from the semantics card (Lattices.jl:265-340,
Checkerboard.jl:471-515, SSHModels.jl:348-562), M from its block picture (SSHModels.jl:581-640), everything else from
numpy.linalg on the dense matrix.

Layouts are the reference's: sites and bonds 1-based, vectors [site][tau] with tau fastest, per-(bond, tau) tables as
(Nbonds, Ltau) arrays in checkerboard order (Julia's (Ltau x Nbonds) column-major), fields [phonon][tau].
"""
import numpy as np


# ----------------------------------------------------------------------------------------------- tables
def raw_table(norb, L1, L2, L3, definition):
    """1-based (isite, fsite) pairs of ONE bond definition (o1, o2, (d1, d2, d3)), cell order, duplicates dropped
    (a wrap bond that coincides with an earlier bond, in either orientation: Lattices.jl:296-313)."""
    o1, o2, d = definition[0], definition[1], tuple(definition[2]) + (0,) * (3 - len(definition[2]))
    seen, have = [], set()
    for cell in range(L1 * L2 * L3):
        l1, l2, l3 = cell % L1, (cell // L1) % L2, cell // (L1 * L2)
        m1, m2, m3 = (l1 + d[0]) % L1, (l2 + d[1]) % L2, (l3 + d[2]) % L3
        p = (norb * cell + o1, norb * (m1 + L1 * m2 + L1 * L2 * m3) + o2)
        if p in have or (p[1], p[0]) in have:
            continue
        have.add(p)
        seen.append(p)
    return np.array(seen, dtype=np.int64).reshape(-1, 2)


def checkerboard_order(table):
    """Orient (smaller site first), stable sort by the key max*i + j, greedy colouring in that order, stable sort by colour.
    Returns (final table, colours in final order, checkerboard_perm 1-based: raw bond -> checkerboard position)."""
    nb = table.shape[0]
    t = np.sort(table, axis=1)
    perm = np.argsort(t.max() * t[:, 0] + t[:, 1], kind="stable")
    t = t[perm]
    colour = np.zeros(nb, dtype=np.int64)
    g = 0
    while (colour == 0).any():
        g += 1
        used = set()
        for n in range(nb):
            if colour[n]:
                continue
            i, j = int(t[n, 0]), int(t[n, 1])
            if i in used or j in used:
                continue
            colour[n] = g
            used.add(i)
            used.add(j)
    new_perm = np.argsort(colour, kind="stable")
    cb_perm = np.argsort(perm[new_perm], kind="stable") + 1
    return t[new_perm], colour[new_perm], cb_perm


class Tables:
    """The integer set-up of an SSH model: definitions = [(o1, o2, (d1, d2, d3), has_phonon), ...] in deck order."""

    def __init__(self, norb, L1, L2, L3, definitions):
        self.N = norb * L1 * L2 * L3
        raws = [raw_table(norb, L1, L2, L3, d) for d in definitions]
        self.per_definition = [r.shape[0] for r in raws]
        self.raw = np.concatenate(raws, axis=0)
        self.Nbonds = self.raw.shape[0]
        p2b, off = [], 0
        for r, d in zip(raws, definitions):
            if d[3]:
                p2b += list(range(off + 1, off + r.shape[0] + 1))            # 1-based raw bond of each phonon (SSHModels.jl:413)
            off += r.shape[0]
        self.phonon_to_bond = np.array(p2b, dtype=np.int64)
        self.Nph = len(p2b)
        self.table, self.colours, self.cb_perm = checkerboard_order(self.raw)
        self.ncolours = int(self.colours.max())
        self.cb_index = self.cb_perm[self.phonon_to_bond - 1] - 1             # 0-based checkerboard position of each phonon's bond
        self.bond_to_phonon_cb = np.zeros(self.Nbonds, dtype=np.int64)        # 1-based phonon on each checkerboard bond, 0 = bare
        self.bond_to_phonon_cb[self.cb_index] = np.arange(1, self.Nph + 1)


def effective_hopping(tab, t, alpha, alpha2, x, Ltau):
    """t' = t - (alpha x + sign(x) alpha2 x^2) per (phonon, tau) (SSHModels.jl:528); t per RAW bond, alpha, alpha2 per phonon."""
    X = np.asarray(x).reshape(tab.Nph, Ltau)
    a, a2 = np.asarray(alpha)[:, None], np.asarray(alpha2)[:, None]
    quad = a2 * X ** 2 if np.iscomplexobj(X) else np.sign(X) * a2 * X ** 2      # (complex x: alpha2 = 0 is the caller's business)
    return np.asarray(t)[tab.phonon_to_bond - 1][:, None] - (a * X + quad)


def hopping_tables(tab, t, alpha, alpha2, x, Ltau, dtau):
    """(cosht, sinht), each (Nbonds, Ltau) in checkerboard order: cosh / sinh(dtau t') on phonon bonds, cosh / sinh(dtau t) on
    bare ones (SSHModels.jl:450-464, 518-535)."""
    tp = effective_hopping(tab, t, alpha, alpha2, x, Ltau)
    tcb = np.empty((tab.Nbonds, Ltau), dtype=tp.dtype)
    tcb[tab.cb_perm - 1] = np.asarray(t)[:, None]
    tcb[tab.cb_index] = tp
    return np.cosh(dtau * tcb), np.sinh(dtau * tcb)


# ----------------------------------------------------------------------------------------------- dense matrices
def dense_cb(N, table, c, s):
    """Dense N x N checkerboard matrix B_nb ... B_2 B_1 (bond 1 acts first) for one time slice."""
    CB = np.eye(N, dtype=np.result_type(c, s))
    for n in range(table.shape[0]):
        i, j = table[n, 0] - 1, table[n, 1] - 1
        ri, rj = CB[i].copy(), CB[j].copy()
        CB[i] = c[n] * ri + s[n] * rj
        CB[j] = c[n] * rj + s[n] * ri
    return CB


def dense_M(tab, Ltau, cosht, sinht, expDtauMu):
    """M[t,t] = 1, M[t,t-1] = -B(t), M[0,L-1] = +B(0), B(t) = CB_t diag(exp(dtau mu)); row/col index = site*Ltau + tau."""
    N = tab.N
    M = np.eye(N * Ltau, dtype=np.result_type(cosht, sinht))
    rows = np.arange(N) * Ltau
    for tau in range(Ltau):
        B = dense_cb(N, tab.table, cosht[:, tau], sinht[:, tau]) * np.asarray(expDtauMu)[None, :]
        M[np.ix_(rows + tau, rows + (tau - 1) % Ltau)] += (1.0 if tau == 0 else -1.0) * B
    return M


def dense_dMdx(tab, Ltau, dtau, cosht, sinht, expDtauMu, alpha, alpha2, x, u, v):
    """d[field] = u^T (dM/dx_field) v for every field, with dM/dx formed densely: for the phonon on checkerboard bond n at slice tau,
    dCB_tau/dx = (B_nb ... B_{n+1}) dB_n/dx (B_{n-1} ... B_1) from dense prefix / suffix products, dB_n/dx the 2 x 2 block
    dtau dt'/dx [[sinh, cosh], [cosh, sinh]](dtau t') with dt'/dx = -(alpha + 2 alpha2 x): SSHModels.jl:803, i.e. WITHOUT the
    sign(x) that update_model! puts in front of alpha2 x^2 (:528) — the reference's quirk, followed here; for alpha2 != 0 and x < 0
    this is not the derivative of M."""
    N, nb = tab.N, tab.Nbonds
    X = np.asarray(x).reshape(tab.Nph, Ltau)
    U, V = np.asarray(u).reshape(N, Ltau), np.asarray(v).reshape(N, Ltau)
    d = np.zeros((tab.Nph, Ltau))
    for tau in range(Ltau):
        c, s = cosht[:, tau], sinht[:, tau]
        w = np.asarray(expDtauMu) * V[:, (tau - 1) % Ltau]
        sign = 1.0 if tau == 0 else -1.0
        P = np.eye(N)                                            # prefix: B_{n-1} ... B_1 when bond n is visited
        S = dense_cb(N, tab.table, c, s)                         # suffix: B_nb ... B_{n+1}, peeled off the full product with B_n^-1
        for n in range(nb):
            i, j = tab.table[n] - 1
            Si, Sj = S[:, i].copy(), S[:, j].copy()              # B_n^-1 = [[cosh, -sinh], [-sinh, cosh]]
            S[:, i], S[:, j] = c[n] * Si - s[n] * Sj, c[n] * Sj - s[n] * Si
            ph = tab.bond_to_phonon_cb[n]
            if ph != 0:
                ij = [i, j]
                dtp = -(alpha[ph - 1] + 2.0 * alpha2[ph - 1] * X[ph - 1, tau])
                dB = dtau * dtp * np.array([[s[n], c[n]], [c[n], s[n]]])
                dCB = S[:, ij] @ dB @ P[ij, :]                   # dense N x N
                d[ph - 1, tau] = sign * (U[:, tau] @ dCB @ w)
            Pi, Pj = P[i].copy(), P[j].copy()
            P[i], P[j] = c[n] * Pi + s[n] * Pj, c[n] * Pj + s[n] * Pi
    return d.reshape(-1)


class DenseSSH:
    """Everything the tests compare against, from numpy.linalg on the dense M of one field configuration."""

    def __init__(self, tab, Ltau, dtau, t, alpha, alpha2, mu, x):
        self.tab, self.Ltau, self.dtau = tab, Ltau, dtau
        self.t, self.alpha, self.alpha2, self.mu = (np.asarray(a, dtype=np.float64) for a in (t, alpha, alpha2, mu))
        self.expDtauMu = np.exp(dtau * self.mu)
        self.set_x(x)

    def set_x(self, x):
        self.x = np.array(x, dtype=np.float64)
        self.cosht, self.sinht = hopping_tables(self.tab, self.t, self.alpha, self.alpha2, self.x, self.Ltau, self.dtau)
        self.M = dense_M(self.tab, self.Ltau, self.cosht, self.sinht, self.expDtauMu)
        self.A = self.M.T @ self.M

    def solve(self, b):
        """x with MtM x = b."""
        return np.linalg.solve(self.A, b)

    def action(self, bp, bm):
        """S_f = sum over the two pseudo-fermion vectors of b . (MtM)^-1 b / 2 (HMC.jl:768-784 with Lambda = 1)."""
        return sum(0.5 * (b @ self.solve(b)) for b in (bp, bm))

    def dMdx(self, u, v):
        return dense_dMdx(self.tab, self.Ltau, self.dtau, self.cosht, self.sinht, self.expDtauMu, self.alpha, self.alpha2, self.x, u, v)

    def force(self, bp, bm):
        """dS_f/dx as the reference defines it (HMC.jl:790-814): -sum_± (M X±)^T dM/dx X±, X± = (MtM)^-1 b±; returns (F, S_f)."""
        F, Sf = np.zeros(self.tab.Nph * self.Ltau), 0.0
        for b in (bp, bm):
            X = self.solve(b)
            Sf += 0.5 * (b @ X)
            F -= self.dMdx(self.M @ X, X)
        return F, Sf


def complex_step_gradient(tab, Ltau, dtau, t, alpha, mu, x, bp, bm, step=1e-30):
    """dS_f/dx from the DEFINITION of the derivative, for alpha2 = 0 (then M is analytic in x): Im S_f(x + i step e_k) / step with
    the dense complex M — no force formula enters."""
    x = np.asarray(x, dtype=np.float64)
    Emu, zero = np.exp(dtau * np.asarray(mu)), np.zeros(tab.Nph)
    out = np.empty(x.size)
    for k in range(x.size):
        xc = x.astype(complex)
        xc[k] += 1j * step
        c, s = hopping_tables(tab, t, alpha, zero, xc, Ltau, dtau)
        M = dense_M(tab, Ltau, c, s, Emu)
        A = M.T @ M
        out[k] = sum(0.5 * (b @ np.linalg.solve(A, b)) for b in (bp, bm)).imag / step
    return out


# ----------------------------------------------------------------------------------------------- phonon action, acceleration, leapfrog
def phonon_action(x, Nph, Ltau, dtau, omega, omega4):
    X = x.reshape(Nph, Ltau)
    return dtau * np.sum(omega[:, None] ** 2 * X ** 2 / 2 + omega4[:, None] * X ** 4 + (X - np.roll(X, 1, axis=1)) ** 2 / dtau ** 2 / 2)


def phonon_action_gradient(x, Nph, Ltau, dtau, omega, omega4):
    X = x.reshape(Nph, Ltau)
    g = dtau * (omega[:, None] ** 2 * X + 4.0 * omega4[:, None] * X ** 3) + (2.0 * X - np.roll(X, 1, axis=1) - np.roll(X, -1, axis=1)) / dtau
    return g.reshape(-1)


def accelerator_mass(Ltau, dtau, omega, m0=1.0, c=0.3):
    """element_Mi of the Fourier accelerator (FourierAccelerators.jl), per (phonon, frequency)."""
    k = np.arange(Ltau)
    kp = np.minimum(k, Ltau - k)
    mreg = m0 * np.exp(-(c * kp / Ltau) ** 2)
    return dtau * (mreg[None, :] ** 2 + omega[:, None] ** 2 + (2 - 2 * np.cos(2 * np.pi * kp / Ltau))[None, :] / dtau ** 2) \
        / (mreg[None, :] ** 2 + omega[:, None] ** 2)


def accelerate(vec, faM, power):
    return np.real(np.fft.ifft(faM ** power * np.fft.fft(vec.reshape(faM.shape), axis=1), axis=1)).reshape(-1)


def dense_leapfrog(D, omega, omega4, faM, x0, R, Rp, Rm, dt, nt):
    """One standard HMC trajectory (HMC.jl:343-463 for the ORDER of the steps only; alpha = 0: full momentum refresh) with exact
    dense solves and the reference's force (DenseSSH.force + the phonon action's gradient).  D is left at the end point.
    Returns dict(x1, v1, v_init, H0, H1, H0_closed)."""
    Nph, L, dtau = D.tab.Nph, D.Ltau, D.dtau
    Sb = lambda x: phonon_action(x, Nph, L, dtau, omega, omega4)
    x = np.array(x0, dtype=np.float64)
    D.set_x(x)
    v = accelerate(R, faM, -0.5)
    v_init = v.copy()
    phis = (D.M.T @ Rp, D.M.T @ Rm)
    K = lambda v: 0.5 * (v @ accelerate(v, faM, 1.0))
    H0 = Sb(x) + D.action(*phis) + K(v)
    Q = accelerate(D.force(*phis)[0] + phonon_action_gradient(x, Nph, L, dtau, omega, omega4), faM, -1.0)
    for _ in range(nt):
        v = v - dt / 2 * Q
        x = x + dt * v
        D.set_x(x)
        Q = accelerate(D.force(*phis)[0] + phonon_action_gradient(x, Nph, L, dtau, omega, omega4), faM, -1.0)
        v = v - dt / 2 * Q
    H1 = Sb(x) + D.action(*phis) + K(v)
    return dict(x1=x, v1=v, v_init=v_init, H0=H0, H1=H1, H0_closed=0.5 * (Rp @ Rp + Rm @ Rm) + Sb(np.asarray(x0)) + K(v_init))


# ----------------------------------------------------------------------------------------------- KPM polynomial
def dense_kpm_apply(tab, Ltau, cosht, sinht, expDtauMu, lam_lo, lam_hi, orders, coeffs, vin):
    """The symmetric KPM preconditioner as dense matrices (KPMPreconditioners.jl:355-481, 606-679): A = CBbar diag(exp(dtau mu)) with
    the tau-MEANS of the per-(bond, tau) cosh / sinh tables, A' = (A - avg)/mag; per frequency w of the twisted transform
    out_w = [sum_m c_m T_m(A')] [sum_m conj(c_m) T_m(A'^T)] nu_w, mirrored to L-1-w by conjugation.  coeffs[w]: complex, orders[w] long."""
    N, L = tab.N, Ltau
    A = dense_cb(N, tab.table, cosht.mean(axis=1), sinht.mean(axis=1)) * np.asarray(expDtauMu)[None, :]
    avg, mag = (lam_hi + lam_lo) / 2, (lam_hi - lam_lo) / 2
    Ap, ApT = (A - avg * np.eye(N)) / mag, (A.T - avg * np.eye(N)) / mag

    def series(Amat, c, vec):
        Tm1, T = vec, Amat @ vec
        out = c[0] * Tm1
        if len(c) > 1:
            out = out + c[1] * T
        for m in range(2, len(c)):
            Tm1, T = T, 2 * (Amat @ T) - Tm1
            out = out + c[m] * T
        return out

    theta = np.exp(-1j * np.pi * np.arange(L) / L)
    nu = np.fft.fft(theta[None, :] * np.asarray(vin).reshape(N, L), axis=1)
    out = np.zeros((N, L), dtype=complex)
    for w in range((L + 1) // 2):
        c = np.asarray(coeffs[w])[:orders[w]]
        uw = series(Ap, c, series(ApT, np.conj(c), nu[:, w]))
        out[:, w] = uw
        out[:, L - 1 - w] = np.conj(uw)
    return np.real(np.conj(theta)[None, :] * np.fft.ifft(out, axis=1)).reshape(-1)
