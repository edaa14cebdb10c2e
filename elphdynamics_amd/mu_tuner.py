"""Host-side mirror of MuFinder.jl: the chemical-potential tuner that steers <N> to a target density while the run goes on.

    tuner = MuTuner(active, init_mu, target_N, N, beta, dtau, forgetful_c, kappa_min, logfile)      MuFinder.jl:15-64
    tuner = from_params(sim.mu_tuner, logfile)                     from what process_input.initialize_mutuner read of [tune_density]
    update_mu_(tuner, N, Nsqr) -> mu                               :117-169   one step from one measurement of <N>, <N^2>
    estimate_mu(tuner)                                             :175-203   tuner.mu_avg, tuner.mu_err from the history
    forgetful_mean, forgetful_welfords                             :212-262   running mean / deviation over the last fraction c
    density_moments(model, Gr, nchains=1) -> (N, Nsqr)             the measurement itself, on the device (elph_density_moments)
    tune_mu_(model, tuner, Gr, hmc=None) -> mu                     :69-112    update_mu!(model, tuner, estimator), one configuration
    tune_mu_chains_(model, tuners, Gr, mu, hmc=None) -> mu         the same for every resident chain, a tuner per chain

The step: with the running means mu_bar, N_bar, Nsqr_bar over the last fraction forgetful_c of the history, the compressibility estimate
kappa_bar = beta (Nsqr_bar - N_bar^2), held between kappa_min / sqrt(n) and sqrt(var N) / std(mu), gives
mu = mu_bar + (target_N - N_bar) / kappa_bar.  N counts electrons of the whole lattice (target_N = density * Nsites, kappa_min is the
deck's value times Nsites); the log file holds per-site values where the reference's does.

The reference measures <N> and <N^2> through setup!(estimator, i, j) for every pair of vectors; here one device call returns them for
all resident chains from the vectors the estimator already holds (csrc/density_moments.hip), so a tuner step costs one pass over R and
M^-1 R.  The drivers take the step after an update of the field and of the estimator (greens.update_), as RunSimulation.jl does after
every update; no run loop is part of this module.
"""
import math
import os

import numpy as np

from . import hmc as _hmc
from ._chain_unit import chain_rows
from ._lib import check, dptr

LOG_HEADER = "mu_bar kappa_bar n_bar Nsqr_bar mu n Nsqr\n"


class MuTuner:
    """MuTuner{T} (MuFinder.jl:15-64): the fields of the reference under ASCII names (mu for μ, Nsqr for N², kappa for κ)."""

    def __init__(self, active, init_mu, target_N, N, beta, dtau, forgetful_c, kappa_min, logfile=""):
        init_mu = float(init_mu)
        self.active = bool(active)
        self.mu_traj = [init_mu]
        self.N_traj = []
        self.Nsqr_traj = []
        self.forgetful_c = float(forgetful_c)
        self.mu = init_mu
        self.N = int(N)
        self.beta = float(beta)
        self.dtau = float(dtau)
        self.L = int(round(self.beta / self.dtau))
        self.target_N = float(target_N)
        self.mu_bar = init_mu
        self.mu_std = 0.0
        self.kappa_bar = float(kappa_min)
        self.N_bar = -1.0
        self.N_std = 0.0
        self.Nsqr_bar = -1.0
        self.mu_bar_traj = []
        self.kappa_bar_traj = []
        self.N_bar_traj = []
        self.Nsqr_bar_traj = []
        self.kappa_min = float(kappa_min)
        self.mu_avg = init_mu
        self.mu_err = 0.0
        self.logfile = str(logfile)
        if self.active and not os.path.isfile(self.logfile):           # a resumed run appends to the log it finds (:55-59)
            with open(self.logfile, "w") as f:
                f.write(LOG_HEADER)


def from_params(params, logfile=""):
    """The tuner of process_input.initialize_mutuner's parameters (ProcessInputFile.jl:611-624); the reference's log file is
    <datafolder>/mu_tuner_log.out, and with chains in lockstep every chain's tuner wants a file of its own."""
    return MuTuner(params.active, params.mu0, params.N_target, params.nsites, params.beta, params.dtau, params.memory, params.kappa_min,
                   logfile if params.active else "")


def _window_starts(n, c):
    """1-based first index of the window over the last fraction c of a history of n - 1 and of n entries."""
    return 1 + math.floor((1.0 - c) * (n - 1)), 1 + math.floor((1.0 - c) * n)


def forgetful_mean(x, prev_mean, c):
    """The mean of the last fraction c of x from the mean before x[-1] was pushed (:212-229): the new entry comes in, and when the window's
    start moved, the entry that left goes out."""
    n_all = len(x)
    if n_all == 1:
        return x[0]
    i_old, i_new = _window_starts(n_all, c)
    n = n_all - i_old + 1
    mean = prev_mean + (x[-1] - prev_mean) / n
    if i_new != i_old:
        n = n_all - i_new + 1
        mean = mean - (x[i_old - 1] - mean) / n
    return mean


def forgetful_welfords(x, prev_mean, prev_std, c):
    """(mean, standard deviation) of the last fraction c of x by Welford's update, entries leaving the window taken out again (:235-262)."""
    n_all = len(x)
    if n_all == 1:
        return x[0], 0.0
    i_old, i_new = _window_starts(n_all, c)
    n = n_all - i_old + 1
    m2 = (n - 2) * prev_std ** 2
    mean = prev_mean + (x[-1] - prev_mean) / n
    m2 = m2 + (x[-1] - mean) * (x[-1] - prev_mean)
    if i_new != i_old:
        n = n_all - i_new + 1
        gone, before = x[i_old - 1], mean
        mean = before - (gone - before) / n
        m2 = m2 - (gone - mean) * (gone - before)
    std = math.sqrt(m2 / (n - 1)) if n > 1 else 0.0
    return mean, std


def update_mu_(tuner, N, Nsqr):
    """One step of the tuner from a new measurement of <N> and <N^2>; returns the new mu (:117-169)."""
    t = tuner
    N, Nsqr = float(N), float(Nsqr)
    t.N_traj.append(N)
    t.Nsqr_traj.append(Nsqr)
    t.mu_bar, t.mu_std = forgetful_welfords(t.mu_traj, t.mu_bar, t.mu_std, t.forgetful_c)
    t.N_bar = forgetful_mean(t.N_traj, t.N_bar, t.forgetful_c)
    t.Nsqr_bar = forgetful_mean(t.Nsqr_traj, t.Nsqr_bar, t.forgetful_c)
    t.mu_bar_traj.append(t.mu_bar)
    t.N_bar_traj.append(t.N_bar)
    t.Nsqr_bar_traj.append(t.Nsqr_bar)
    n = len(t.N_traj)
    var_N = t.Nsqr_bar - t.N_bar ** 2
    kappa_lo = t.kappa_min / math.sqrt(n)
    if n == 1 or var_N < 0.0 or t.mu_std <= 0.0:
        kappa_hi = kappa_lo
    else:
        kappa_hi = math.sqrt(var_N) / t.mu_std
    t.kappa_bar = max(min(t.beta * var_N, kappa_hi), kappa_lo)      # the upper bound first, then the lower one
    t.kappa_bar_traj.append(t.kappa_bar)
    if t.active:
        with open(t.logfile, "a") as f:
            f.write("%.8f %.8f %.8f %.8f %.8f %.8f %.8f\n" % (t.mu_bar, t.kappa_bar / t.N, t.N_bar / t.N, t.Nsqr_bar, t.mu, N / t.N, Nsqr))
    t.mu = t.mu_bar + (t.target_N - t.N_bar) / t.kappa_bar
    t.mu_traj.append(t.mu)
    return t.mu


def estimate_mu(tuner):
    """The best guess of mu and its error from the history into tuner.mu_avg, tuner.mu_err (:175-203): mu_bar, and the deviation of the
    window's mu about its median; a tuner that uses its whole history (forgetful_c = 1) judges the error from the last half."""
    t = tuner
    if not t.active:
        t.mu_avg, t.mu_err = t.mu, 0.0
        return
    c = 0.5 if t.forgetful_c == 1.0 else t.forgetful_c
    first = math.ceil(c * len(t.mu_traj))                           # 1-based
    window = np.asarray(t.mu_traj[first - 1:], dtype=np.float64)
    dev = window - np.median(window)
    t.mu_avg = t.mu_bar
    t.mu_err = math.sqrt(float(np.sum(dev * dev)) / (window.size - 1)) if window.size > 1 else float("nan")


def density_moments(model, Gr, nchains=1):
    """(<N>[nchains], <N^2>[nchains]) of the chains resident in the model from the vectors the estimator holds (greens.update_ or
    greens.set_vectors_ first): elph_density_moments, one device call for all chains."""
    assert Gr.model is model
    nchains = int(nchains)
    N, Nsqr = np.zeros(nchains), np.zeros(nchains)
    check(model._lib.elph_density_moments(model._h, nchains, dptr(N), dptr(Nsqr)))
    return N, Nsqr


def tune_mu_(model, tuner, Gr, hmc=None):
    """update_mu!(model, tuner, estimator) (:69-112) for one configuration: measure, step, shift every site's model.mu by the step's
    change of the mean; returns the new mean.  With a dynamics state `hmc` its device copy follows (hmc.set_mu_); without one the
    caller's next models.update_model_ takes model.mu.  An inactive tuner records mean(model.mu) and touches nothing."""
    mu0 = float(np.mean(model.mu))
    if not tuner.active:
        tuner.mu = mu0
        return mu0
    N, Nsqr = density_moments(model, Gr, 1)
    mu1 = update_mu_(tuner, N[0], Nsqr[0])
    model.mu += mu1 - mu0
    tuner.mu = mu1
    if hmc is not None:
        _hmc.set_mu_(model, hmc, model.mu)
    return mu1


def tune_mu_chains_(model, tuners, Gr, mu, hmc=None):
    """tune_mu_ for every resident chain, a tuner per chain: one measurement call for all chains, one step per tuner, row c of mu
    ((nchains, Nsites)) shifted by chain c's step, and one hmc.set_mu_ (elph_hmc_set_mu_chains) for the dynamics state when given.
    Returns mu (float64, C-contiguous: the caller's array when it is that already) for chain_measurements.accumulate_(..., mu=mu) or
    its SSH twin.  An inactive tuner records its row's mean and leaves the row."""
    nch = len(tuners)
    out = chain_rows(mu, nch, model.Nsites, "mu")
    if not any(t.active for t in tuners):
        for c, t in enumerate(tuners):
            t.mu = float(np.mean(out[c]))
        return out
    N, Nsqr = density_moments(model, Gr, nch)
    for c, t in enumerate(tuners):
        mu0 = float(np.mean(out[c]))
        if t.active:
            mu1 = update_mu_(t, N[c], Nsqr[c])
            out[c] += mu1 - mu0
            t.mu = mu1
        else:
            t.mu = mu0
    if hmc is not None:
        _hmc.set_mu_(model, hmc, out)
    return out
