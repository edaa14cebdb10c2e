"""The chemical-potential tuner's host side (elphdynamics_amd/mu_tuner.py, the mirror of MuFinder.jl) without a device: the forgetful
running statistics against plain window statistics, the first step's closed form, the bounds on kappa, a closed loop on a linear
response with noise, the log file, and the tuner built from a deck's [tune_density] parameters."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from elphdynamics_amd import mu_tuner as mt

DECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decks")


def window_start(n, c):
    """0-based first index of the window over the last fraction c of n entries: i = 1 + floor((1 - c) n), 1-based."""
    return math.floor((1.0 - c) * n)


@pytest.mark.parametrize("c", [1.0, 0.75, 0.5, 0.3])
def test_forgetful_statistics_equal_the_plain_statistics_of_the_window(c):
    rng = np.random.default_rng(7)
    x, mean_w, std_w, mean_m = [], 0.0, 0.0, 0.0
    worst = 0.0
    for v in 1.5 + rng.standard_normal(200):
        x.append(float(v))
        mean_w, std_w = mt.forgetful_welfords(x, mean_w, std_w, c)
        mean_m = mt.forgetful_mean(x, mean_m, c)
        win = np.array(x[window_start(len(x), c):])
        want_std = win.std(ddof=1) if win.size > 1 else 0.0
        worst = max(worst, abs(mean_w - win.mean()), abs(mean_m - win.mean()), abs(std_w - want_std))
    print("c = %g: worst deviation %.2e" % (c, worst))
    assert worst <= 1e-12


def make(tmp_path, name="log.out", **kw):
    par = dict(active=True, init_mu=-0.25, target_N=12.0, N=16, beta=4.0, dtau=0.1, forgetful_c=0.75, kappa_min=1.6)
    par.update(kw)
    return mt.MuTuner(logfile=str(tmp_path / name), **par)


def test_first_step_closed_form_trajectory_lengths_and_kappa_bounds(tmp_path):
    t = make(tmp_path)
    assert t.L == 40 and t.mu_traj == [-0.25] and t.kappa_bar == 1.6 and t.N_bar == -1.0 and t.Nsqr_bar == -1.0
    mu1 = mt.update_mu_(t, 11.0, 123.0)
    assert mu1 == -0.25 + (12.0 - 11.0) / 1.6 == t.mu                       # n = 1: kappa_bar = kappa_min, mu_bar = mu_0, N_bar = N
    assert t.mu_std == 0.0 and t.kappa_bar == 1.6 and t.mu_bar == -0.25 and t.N_bar == 11.0 and t.Nsqr_bar == 123.0

    def lengths():
        return [len(a) for a in (t.mu_traj, t.N_traj, t.Nsqr_traj, t.mu_bar_traj, t.kappa_bar_traj, t.N_bar_traj, t.Nsqr_bar_traj)]
    assert lengths() == [2, 1, 1, 1, 1, 1, 1]
    rng = np.random.default_rng(3)
    for n in range(2, 40):
        N = 12.0 + rng.standard_normal()
        mt.update_mu_(t, N, N * N + 2.0 * rng.random() - 0.5)               # var N of either sign: every branch of the upper bound
        assert lengths() == [n + 1] + [n] * 6
        if n == 3:
            assert lengths() == [4, 3, 3, 3, 3, 3, 3]
        lo = t.kappa_min / math.sqrt(n)
        var_N = t.Nsqr_bar - t.N_bar ** 2
        hi = lo if (var_N < 0.0 or t.mu_std <= 0.0) else math.sqrt(var_N) / t.mu_std
        assert lo <= t.kappa_bar <= max(lo, hi), (n, lo, t.kappa_bar, hi)
        assert t.kappa_bar == max(min(t.beta * var_N, hi), lo)
        assert t.mu == t.mu_traj[-1] == t.mu_bar + (t.target_N - t.N_bar) / t.kappa_bar


@pytest.mark.parametrize("c", [0.75, 1.0])
def test_closed_loop_on_a_linear_response_converges_within_the_bound_of_its_noise(tmp_path, c):
    """The system: N(mu) = N* + kappa* (mu - mu*) + eps, N^2 = N^2 + kappa* / beta + eta, eps ~ N(0, sigma^2), eta ~ N(0, sigma_eta^2).

    The bound.  Write d_n = mu_n - mu*.  The windows of mu_traj and of N_traj hold the same steps, so N_bar - N* = kappa* D_n + e_n with
    D_n the window's mean of d and e_n the window's mean of eps, and the step mu_n = mu_bar + (N* - N_bar) / kappa_bar is exactly
        d_n = a_n D_n - e_n / kappa_bar_n,      a_n = 1 - kappa* / kappa_bar_n.
    While 2/3 kappa* <= kappa_bar_n <= 2 kappa*, |a_n| <= A = 1/2 and 1 / kappa_bar_n <= 3 / (2 kappa*).  This premise is asserted at every
    step; it holds because kappa_min = kappa* keeps the lower bound at or under kappa*, N^2 is built so that beta var N = kappa* + beta
    (window variance of N), and the parameters keep the latter small: beta sigma^2 = 0.16 and beta kappa*^2 d_0^2 / n = 10.2 / n against
    kappa* = 8.  |D_n| <= the window's mean of |d_k|, so by induction |d_n| <= B_n with
        B_0 = |d_0|,      B_n = A mean_window(B_k) + 3 |e_n| / (2 kappa*),
    and after the last step |mu_bar - mu*| = |D| <= mean_window(B_k).  B is computed below from the noise the test drew and the window
    rule alone (nothing of the tuner's state enters); it ends at 6e-3 (c = 0.75) and 2e-2 (c = 1), a tenth of the initial error d_0 = 0.2 or less."""
    beta, kappa, mu_star, N_star, sigma, sigma_eta, steps = 4.0, 8.0, -0.3, 12.0, 0.2, 0.01, 400
    t = make(tmp_path, init_mu=mu_star + 0.2, target_N=N_star, beta=beta, forgetful_c=c, kappa_min=kappa)
    rng = np.random.default_rng(11)
    eps, eta = sigma * rng.standard_normal(steps), sigma_eta * rng.standard_normal(steps)
    B = [0.2]
    for n in range(1, steps + 1):
        N = N_star + kappa * (t.mu - mu_star) + eps[n - 1]
        mt.update_mu_(t, N, N * N + kappa / beta + eta[n - 1])
        assert 2.0 / 3.0 * kappa <= t.kappa_bar <= 2.0 * kappa, (n, t.kappa_bar)          # the premise of the bound
        i0 = window_start(n, c)
        B.append(0.5 * np.mean(B[i0:n]) + 1.5 * abs(eps[i0:n].mean()) / kappa)
        assert abs(t.mu - mu_star) <= B[n] * (1 + 1e-9), (n, t.mu - mu_star, B[n])
    bound = float(np.mean(B[window_start(steps, c):steps]))
    print("c = %g: |mu_bar - mu*| = %.3e, bound %.3e; kappa_bar = %.3f" % (c, abs(t.mu_bar - mu_star), bound, t.kappa_bar))
    assert bound < 0.2 / 4                                                  # the bound says something: well inside the initial error
    assert abs(t.mu_bar - mu_star) <= bound
    mt.estimate_mu(t)
    assert t.mu_avg == t.mu_bar and t.mu_err > 0.0
    first = math.ceil((0.5 if c == 1.0 else c) * len(t.mu_traj))            # forgetful_c = 1: the last half
    win = np.array(t.mu_traj[first - 1:])
    assert win.size == len(t.mu_traj) - first + 1
    want = math.sqrt(np.sum((win - np.median(win)) ** 2) / (win.size - 1))
    assert abs(t.mu_err - want) <= 1e-15 + 1e-12 * want


def test_inactive_tuner_returns_the_mean_and_writes_nothing(tmp_path):
    t = make(tmp_path, active=False)
    assert not os.path.exists(t.logfile)
    model = SimpleNamespace(mu=np.array([0.1, 0.2, 0.6]))
    got = mt.tune_mu_(model, t, None)                                       # no estimator is touched
    assert got == t.mu == float(np.mean(model.mu)) and np.array_equal(model.mu, [0.1, 0.2, 0.6])
    assert t.mu_traj == [-0.25] and t.N_traj == [] and t.kappa_bar_traj == []
    mu = np.array([[0.1, 0.3], [0.5, 0.9]])
    ts = [make(tmp_path, name="a.out", active=False), make(tmp_path, name="b.out", active=False)]
    out = mt.tune_mu_chains_(SimpleNamespace(Nsites=2), ts, None, mu)
    assert out is mu and np.array_equal(mu, [[0.1, 0.3], [0.5, 0.9]]) and [x.mu for x in ts] == [float(np.mean(r)) for r in mu]
    mt.estimate_mu(t)
    assert t.mu_avg == t.mu and t.mu_err == 0.0
    assert os.listdir(tmp_path) == []
    with pytest.raises(ValueError, match="nchains, Nsites"):
        mt.tune_mu_chains_(SimpleNamespace(Nsites=3), ts, None, mu)


def test_log_file_header_once_and_one_line_of_eight_decimals_per_step(tmp_path):
    t = make(tmp_path)
    assert open(t.logfile).read() == "mu_bar kappa_bar n_bar Nsqr_bar mu n Nsqr\n"
    mu0 = t.mu
    mt.update_mu_(t, 11.0, 123.0)
    mu1 = t.mu
    mt.update_mu_(t, 12.5, 158.0)
    t2 = make(tmp_path)                                                     # a resumed run opens the same file: no second header
    mt.update_mu_(t2, 12.0, 146.0)
    lines = open(t.logfile).read().splitlines()
    assert len(lines) == 4 and lines[0] == "mu_bar kappa_bar n_bar Nsqr_bar mu n Nsqr" and sum(ln.startswith("mu_bar") for ln in lines) == 1
    for ln in lines[1:]:
        assert len(ln.split()) == 7 and all(len(w.split(".")[1]) == 8 for w in ln.split())
    # the first line: mu_bar, kappa_bar / N, N_bar / N, Nsqr_bar, the mu the measurement was taken at, N / N, Nsqr
    assert lines[1] == "%.8f %.8f %.8f %.8f %.8f %.8f %.8f" % (mu0, 1.6 / 16, 11.0 / 16, 123.0, mu0, 11.0 / 16, 123.0)
    assert lines[2] == "%.8f %.8f %.8f %.8f %.8f %.8f %.8f" % (t.mu_bar_traj[1], t.kappa_bar_traj[1] / 16, t.N_bar_traj[1] / 16,
                                                               t.Nsqr_bar_traj[1], mu1, 12.5 / 16, 158.0)


def test_from_params_of_a_deck_with_and_without_tune_density(tmp_path):
    """No deck under tests/decks/ has the table, so it is added to the parsed deck; the model is a stand-in with the four fields
    initialize_mutuner reads (process_input_file itself needs a device)."""
    from elphdynamics_amd import process_input as pi
    deck = pi.read_deck(os.path.join(DECKS, "holstein_hmc_honeycomb_L3.toml"))
    assert "tune_density" not in deck
    model = SimpleNamespace(mu=np.array([-0.5, -0.3] * 9), Nsites=18, beta=2.0, dtau=0.1)
    log, mean = str(tmp_path / "mu_tuner_log.out"), float(np.mean(model.mu))
    off = mt.from_params(pi.initialize_mutuner(deck, model), log)
    assert not off.active and off.mu == mean and off.target_N == 18.0 and off.forgetful_c == 0.75 and off.kappa_min == 0.1 and off.logfile == ""
    assert not os.path.exists(log)
    deck["tune_density"] = {"density": 0.8, "memory": 0.5, "kappa_min": 0.05}
    par = pi.initialize_mutuner(deck, model)
    on = mt.from_params(par, log)
    assert on.active and on.mu == on.mu_bar == on.mu_avg == par.mu0 == mean and on.mu_traj == [mean]
    assert on.target_N == 0.8 * 18 and on.N == 18 and on.beta == 2.0 and on.dtau == 0.1 and on.L == 20
    assert on.forgetful_c == 0.5 and on.kappa_min == on.kappa_bar == 0.05 * 18 and on.logfile == log
    assert open(log).read() == mt.LOG_HEADER
