"""The draw rule of elph_hmc_special_update_chains (include/elph_gpu.h; SpecialUpdates.jl:113 reflection, :248-258 Holstein swap,
:324-328 SSH swap), restated in numpy over the build's counter-based generator (elphdynamics_amd/synth.py), and the explicit replay
of such a call through special_move_chains_ with every random input built from synth.

Batches per move, in this order: draw, Rp, Rm, [kpm_randn], u.  The draw batch is synth.uniform01(batch seed, 2 nch): chain c takes
u0 = u[2c] and u1 = u[2c + 1]."""
import numpy as np

from elphdynamics_amd import synth

SQRT_EPS = 1.4901161193847656e-08          # sqrt(eps(Float64)): the default rtol of Julia's isapprox

REFLECT, SWAP = 0, 1


def pick(u, n):
    """min(floor(u n), n - 1): uniform01 can round to 1.0."""
    return int(min(np.floor(u * n), n - 1))


def isapprox(a, b):
    """Julia's a ≈ b for vectors: ‖a − b‖₂ ≤ √eps max(‖a‖₂, ‖b‖₂)."""
    return np.sqrt(np.sum((a - b) ** 2)) <= SQRT_EPS * max(np.sqrt(np.sum(a * a)), np.sqrt(np.sum(b * b)))


def different_columns(X, i):
    """D: the columns q, in increasing order, whose world line X[q] is not ≈ X[i].  X: (Nph, Ltau)."""
    return [q for q in range(X.shape[0]) if not isapprox(X[i], X[q])]


def ssh_pair(X, u0, u1):
    """(i, j) of an SSH swap on the field X (Nph, Ltau): i = pick(u0, Nph), j = D[pick(u1, |D|)], j = i when D is empty."""
    i = pick(u0, X.shape[0])
    D = different_columns(X, i)
    return i, (D[pick(u1, len(D))] if D else i)


def draw(kind, ssh, u, nf, fields=None, table=None):
    """The columns (ci[nch], cj[nch], 0-based) the draw batch u (2 nch uniforms) selects.
    Reflection: nf = Nph.  Holstein swap: table (Nbonds, 2) 1-based sites.  SSH swap: fields (nch, Nph * Ltau), tau fastest."""
    nch = len(u) // 2
    ci, cj = np.zeros(nch, dtype=np.int64), np.zeros(nch, dtype=np.int64)
    for c in range(nch):
        u0, u1 = u[2 * c], u[2 * c + 1]
        if kind == REFLECT:
            ci[c] = cj[c] = pick(u0, nf)
        elif not ssh:
            b = pick(u0, table.shape[0])
            ci[c], cj[c] = table[b, 0] - 1, table[b, 1] - 1
        else:
            ci[c], cj[c] = ssh_pair(np.asarray(fields[c]).reshape(nf, -1), u0, u1)
    return ci, cj


class Batches:
    """The handle's batch counter, restated: batch b (1-based) is seeded with synth.batch_seed(seed, b)."""

    def __init__(self, seed, start=0):
        self.seed, self.b = seed, start

    def _next(self):
        self.b += 1
        return synth.batch_seed(self.seed, self.b)

    def uniform(self, n):
        return synth.uniform01(self._next(), n)

    def randn(self, n):
        return synth.randn(self._next(), n)


def apply_move(x, kind, i, j, nf):
    """The proposed move on one chain's flat field (tau fastest): a copy with column i negated / columns i, j exchanged."""
    X = np.array(x, dtype=np.float64).reshape(nf, -1)
    if kind == REFLECT:
        X[i] = -X[i]
    else:
        X[[i, j]] = X[[j, i]]
    return X.reshape(-1)


def replay(model, H, kind, nmoves, seed, with_kpm, P, fields, start=0):
    """The call special_update_(model, H, kind, nmoves) of a handle seeded with `seed`, replayed on the generator-less handle H move by
    move through hmc.special_move_chains_: columns from draw() on the fields as they stand, Rp, Rm, kpm_randn, u from synth for the
    batch numbers the order gives.  fields: (nch, Ndof) the fields H starts from (it is updated from the decisions: the moves only
    permute or negate elements, so no read-back is needed).
    -> dict(col_i, col_j, accepted, S0, S1, iters, flags, u, P: (nmoves, nch) arrays; batches; fields)."""
    from elphdynamics_amd import hmc, models
    nch, ssh = H.nchains, model.kind == models.SSH
    X = np.array(fields, dtype=np.float64).reshape(nch, model.Ndof)
    B = Batches(seed, start)
    out = {k: [] for k in ("col_i", "col_j", "accepted", "S0", "S1", "iters", "flags", "u", "P")}
    for _ in range(nmoves):
        ci, cj = draw(kind, ssh, B.uniform(2 * nch), model.Nph, fields=X, table=model.neighbor_table)
        r = dict(Rp=B.randn(nch * model.Ndim).reshape(nch, model.Ndim), Rm=B.randn(nch * model.Ndim).reshape(nch, model.Ndim))
        r["kpm_randn"] = B.randn(2 * nch * model.Nsites).reshape(2, nch, model.Nsites) if with_kpm else None
        r["u"] = B.uniform(nch)
        acc, s0, s1, it, fl = hmc.special_move_chains_(model, H, kind, ci, cj, P=P, randoms=r)
        for c in range(nch):
            if acc[c]:
                X[c] = apply_move(X[c], kind, ci[c], cj[c], model.Nph)
        for k, v in zip(out, (ci, cj, acc, s0, s1, it, fl, r["u"], np.minimum(1.0, np.exp(-(s1 - s0))))):
            out[k].append(np.array(v))
    out = {k: np.stack(v) for k, v in out.items()}
    out["batches"], out["fields"] = B.b, X
    return out
