"""GPU tests of the estimator's device-drawn update (csrc/greens_noise.hip, elph_greens_set_rng / elph_greens_update_rng through
greens.EstimateGreensFunction.device_rng_ and greens.update_).

Bounds are the project's own for its generator (tests/test_gpu_hmc.py): atol = 1e-12 against synth.randn for device-drawn normals (the
device's log / sincos against numpy's), relative 1e-8 at tol = 1e-9 with iteration counts within 1 for a solve fed the same numbers by the
other route, and 5 sigma on the moments.  Batch b of seed s is synth.randn(synth.batch_seed(s, b), n_v Ndim).reshape(n_v, Ndim): the numbering
of the host array, whatever the kernel's mapping of Box-Muller pairs to threads (site-fastest for even L, pair-indexed for odd L)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EEDFACE


def small_triangular(**kw):
    """configs.make_model("t") with beta = 0.9, dtau = 0.1: N = 9 sites, L = 9 slices — pairs straddle sites and vectors."""
    from elphdynamics_amd import lattice as lat, models, synth
    m = models.HolsteinModel(lat.Lattice(1, 3, 3, 1), 0.9, 0.1, **kw)
    rng = np.random.default_rng(synth.SEED_FIELDS + 991)
    for (o1, o2, d) in lat.TRIANGULAR_BONDS:
        m.assign_t_(1.0, o1, o2, d, stddev=0.0, rng=rng)
    m.assign_omega_(1.0)
    m.assign_lambda_(1.0)
    m.assign_mu_(0.0)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, 0.9, 0.1)
    models.update_model_(m)
    assert m.Nsites == 9 and m.Ltau == 9
    return m


def make(tag, nch=1, **kw):
    from elphdynamics_amd import configs, models, synth
    m = small_triangular(**kw) if tag == "tri9" else configs.make_model(tag, **kw)
    if nch > 1:
        models.update_model_chains_(m, np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=900 + c) for c in range(nch)]))
    return m


def batch(seed, b, nv, ndim):
    from elphdynamics_amd import synth
    return synth.randn(synth.batch_seed(seed, b), nv * ndim).reshape(nv, ndim)


def fetch_R(m, nv):
    from elphdynamics_amd._lib import check, dptr
    R = np.zeros((nv, m.Ndim))
    check(m._lib.elph_greens_get_vectors(m._h, dptr(R), None))
    return R


def batches_of(m):
    n = C.c_uint64(12345)
    assert m._lib.elph_greens_rng_batches(m._h, C.byref(n)) == 0
    return n.value


# ---------------------------------------------------------------------------------------------- 1. numbering

@pytest.mark.parametrize("tag,nch,nv", [("b", 1, 3), ("d", 1, 2), ("e", 1, 2), ("B", 3, 6), ("tri9", 1, 3), ("C", 1, 2)])
def test_device_drawn_vectors_are_the_batches_of_synth_randn(tag, nch, nv):
    """R after each of two device-drawn updates is batch 1, then batch 2, in the host array's numbering (with chains resident vector v of
    chain c is row v nchains + c of that same array).  tri9 is 243 normals: odd L, odd count, the last normal has no partner; C is many
    workgroups with a grid tail in neither direction a multiple of anything but 256."""
    from elphdynamics_amd import greens
    m = make(tag, nch, tol=1e-5)
    try:
        est = greens.EstimateGreensFunction(m, nv=nv)
        est.device_rng_(SEED)
        assert est.device_rng and batches_of(m) == 0
        for b in (1, 2):
            it, res, fl = greens.update_(est, m)
            assert it.shape == res.shape == fl.shape == (nv,) and not fl.any() and (it > 0).all()
            got, want = fetch_R(m, nv), batch(SEED, b, nv, m.Ndim)
            err = np.abs(got - want).max()
            print("%s batch %d: %d normals, largest deviation from synth.randn %.2e (bound 1e-12)" % (tag, b, want.size, err))
            assert np.allclose(got, want, rtol=0, atol=1e-12)
            assert not est.R.any() and not est.MinvR.any()                  # the host mirrors are not filled on this path ...
        assert batches_of(m) == 2
        est.pull_()                                                          # ... until asked for
        assert np.array_equal(est.R, got) and est.MinvR.any()
    finally:
        m.close()


@pytest.mark.parametrize("tag,nvec", [("tri9", 3), ("tri9", 2), ("b", 3), ("C", 2)])
def test_both_mappings_of_the_generator_write_the_same_bits(tag, nvec):
    """The private hook fills a device buffer (layout S, [vec][tau][site]) with either mapping: the pair-indexed one and the shipped one
    agree bit for bit and equal synth.randn; the site-fastest mapping is refused for an odd L."""
    from elphdynamics_amd import synth
    from elphdynamics_amd._lib import ELPH_E_UNSUPPORTED, check, dptr
    m = make(tag)
    try:
        n = nvec * m.Ndim
        out = {}
        for mapping in (0, -1, 1):
            buf, ms = np.zeros(n), C.c_double(-1.0)
            rc = m._lib.elph_bench_greens_noise(m._h, mapping, nvec, 77, 1, C.byref(ms), 0, n, dptr(buf))
            if mapping == 1 and m.Ltau % 2:
                assert rc == ELPH_E_UNSUPPORTED
                continue
            check(rc)
            assert ms.value >= 0.0
            out[mapping] = buf.reshape(nvec, m.Ltau, m.Nsites).transpose(0, 2, 1).reshape(-1)      # -> the reference numbering
        assert all(np.array_equal(out[0], v) for v in out.values())
        assert np.allclose(out[0], synth.randn(77, n), rtol=0, atol=1e-12)
        # a window of the buffer, and the refusal of one that runs past its end
        win = np.zeros(5)
        check(m._lib.elph_bench_greens_noise(m._h, -1, nvec, 77, 2, None, n - 5, 5, dptr(win)))
        assert np.array_equal(win, out[-1].reshape(nvec, m.Nsites, m.Ltau).transpose(0, 2, 1).reshape(-1)[-5:])
        assert m._lib.elph_bench_greens_noise(m._h, -1, nvec, 77, 1, None, n - 4, 5, dptr(win)) == -1
    finally:
        m.close()


def normals_at(seed, n, idx):
    """Elements idx (reference numbering) of synth.randn(seed, n) without the n - len(idx) others: the same arithmetic, by index."""
    from elphdynamics_amd import synth
    idx = np.asarray(idx, dtype=np.uint64)
    m = np.uint64((n + 1) // 2)

    def u01(i):                                                             # synth.uniform01(seed, ...)[i]
        with np.errstate(over="ignore"):
            z = np.uint64(seed & synth._MASK) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        return ((z >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)

    k = idx // np.uint64(2)
    r, th = np.sqrt(-2.0 * np.log(u01(k))), 2.0 * np.pi * u01(m + k)
    return np.where(idx % np.uint64(2) == 0, r * np.cos(th), r * np.sin(th))


def test_more_vectors_than_the_grid_has_rows():
    """70 000 vectors of b: beyond the 65 535 rows of the site-fastest kernel's grid, whose workgroups then stride over the vectors."""
    from elphdynamics_amd import synth
    from elphdynamics_amd._lib import check, dptr
    m = make("b")
    try:
        nvec = 70000
        n = nvec * m.Ndim
        buf = np.zeros(n)
        check(m._lib.elph_bench_greens_noise(m._h, 1, nvec, 3, 1, None, 0, n, dptr(buf)))
        got = buf.reshape(nvec, m.Ltau, m.Nsites).transpose(0, 2, 1).reshape(-1)
        assert np.allclose(got, synth.randn(3, n), rtol=0, atol=1e-12)
    finally:
        m.close()


def test_element_indices_beyond_two_to_the_31():
    """52 430 vectors of C are 2 147 532 800 normals (17 GB): both mappings, read back in two windows of the device buffer, one across
    element 2^31 and one at the very end, agree bit for bit and equal the generator's numbers at those indices."""
    from elphdynamics_amd import synth
    from elphdynamics_amd._lib import check, dptr
    for k in (243, 1000):                                                   # the by-index restatement is synth.randn itself
        assert np.array_equal(normals_at(9, k, np.arange(k)), synth.randn(9, k))
    m = make("C")
    try:
        N, L, per, nvec = m.Nsites, m.Ltau, m.Ndim, 52430
        n = nvec * per
        assert n > 2 ** 31 + 4096
        for first in (2 ** 31 - 2048, n - 4096):
            p = first + np.arange(4096)                                     # layout S: p = vec per + t N + site
            vec, t, site = p // per, (p % per) // N, p % N
            want = normals_at(5, n, vec * per + site * L + t)
            wins = []
            for mapping in (0, 1):
                win = np.zeros(4096)
                check(m._lib.elph_bench_greens_noise(m._h, mapping, nvec, 5, 1, None, int(first), 4096, dptr(win)))
                wins.append(win)
            assert np.array_equal(wins[0], wins[1]) and np.allclose(wins[1], want, rtol=0, atol=1e-12)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------- 2. the same update

@pytest.mark.parametrize("tag,nch,nv,with_kpm", [("b", 1, 3, False), ("B", 3, 6, True)])
def test_device_drawn_update_equals_the_update_handed_the_same_vectors(tag, nch, nv, with_kpm):
    from elphdynamics_amd import greens, preconditioners as pc, synth
    start = dict(b_max=synth.randn(41, nch * 64).reshape(nch, -1), b_min=synth.randn(42, nch * 64).reshape(nch, -1)) if with_kpm else None

    def run(R):
        m = make(tag, nch, tol=1e-9, maxiter=20000)
        try:
            if start is not None:
                assert m.Nsites == 64
            P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0) if with_kpm else None
            est = greens.EstimateGreensFunction(m, nv=nv)
            if R is None:
                est.device_rng_(SEED + 1)
            out = greens.update_(est, m, P, R=R, setup_kwargs=start)
            if R is None:
                est.pull_()
            return out, est.R.copy(), est.MinvR.copy()
        finally:
            m.close()

    (it_a, res_a, fl_a), R_a, X_a = run(None)
    (it_b, res_b, fl_b), R_b, X_b = run(R_a)
    assert np.array_equal(R_a, R_b) and np.allclose(R_a, batch(SEED + 1, 1, nv, R_a.shape[1]), rtol=0, atol=1e-12)
    assert not fl_a.any() and np.array_equal(fl_a, fl_b) and np.all(np.abs(it_a - it_b) <= 1), (it_a, it_b)
    err = np.abs(X_a - X_b).max() / np.abs(X_b).max()
    print("%s: M^-1 R of the two routes differ by %.2e of the largest element (bound 1e-8), iterations %s / %s" % (tag, err, it_a, it_b))
    assert err < 1e-8


# ---------------------------------------------------------------------------------------------- 3. moments

def test_device_drawn_vectors_have_the_right_moments():
    """1.3 M normals as the vectors of one update of C with two chains: mean, variance, fourth moment, and the lag-1 correlations along the
    time axis and along the site axis (the two directions in which the site-fastest mapping places neighbours), at 5 sigma."""
    from elphdynamics_amd import greens
    nch, nv = 2, 16
    m = make("C", nch, tol=1e-5)
    try:
        est = greens.EstimateGreensFunction(m, nv=nv * nch)
        est.device_rng_(20261019)
        greens.update_(est, m)
        v = fetch_R(m, nv * nch).reshape(nv * nch, m.Nsites, m.Ltau)
        n = v.size
        assert n == 1310720
        assert abs(v.mean()) < 5 / np.sqrt(n) and abs(v.var() - 1) < 5 * np.sqrt(2 / n) and abs((v ** 4).mean() - 3) < 5 * np.sqrt(96 / n)
        along_tau, along_site = v[:, :, 1:] * v[:, :, :-1], v[:, 1:, :] * v[:, :-1, :]
        assert abs(along_tau.mean()) < 5 / np.sqrt(along_tau.size) and abs(along_site.mean()) < 5 / np.sqrt(along_site.size)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------- 4. downstream

def test_tuner_and_measurements_read_the_device_drawn_vectors_in_place():
    """B with three chains.  The tuner's <N>, <N^2> after a device-drawn update equal, bit for bit, those of a handle given the fetched
    vectors (density_moments.hip promises the same bits for the same inputs); chain_measurements.make_measurements_ with neither R nor rng
    equals the same call handed the explicit batch as R within 1e-8 of each array's largest element.  tol = 1e-12: the comparison is about
    which vectors are read, so the stop test's own noise (of the order of tol times the condition number) is kept far below the bound."""
    from test_gpu_measurements import ALL_TD, snapshot
    from elphdynamics_amd import chain_measurements as cms, greens, mu_tuner as mt, synth
    nch, nvc = 3, 2
    nv = nch * nvc
    X = np.stack([synth.phonon_field(64, 40, 4.0, 0.1, seed=900 + c) for c in range(nch)])
    ma, mb = make("B", nch, tol=1e-12, maxiter=20000), make("B", nch, tol=1e-12, maxiter=20000)
    try:
        assert X.shape[1] == ma.Ndof
        ea, eb = greens.EstimateGreensFunction(ma, nv=nv), greens.EstimateGreensFunction(mb, nv=nv)
        ea.device_rng_(SEED + 2)
        greens.update_(ea, ma)
        Na, N2a = mt.density_moments(ma, ea, nch)
        ea.pull_()
        greens.set_vectors_(eb, ea.R, ea.MinvR)
        Nb, N2b = mt.density_moments(mb, eb, nch)
        assert np.array_equal(Na, Nb) and np.array_equal(N2a, N2b) and len(set(Na)) == nch
        ca = cms.initialize_chain_measurements_container(ma, dict(ALL_TD, num_random_vectors=nvc), [""] * nch)
        cb = cms.initialize_chain_measurements_container(mb, dict(ALL_TD, num_random_vectors=nvc), [""] * nch)
        out_a = cms.make_measurements_(ca, ma, ea, X, 1)
        out_b = cms.make_measurements_(cb, mb, eb, X, 1, R=batch(SEED + 2, 2, nv, mb.Ndim))
        assert batches_of(ma) == 2
        assert np.array_equal(out_a[2], out_b[2]) and np.all(np.abs(out_a[0] - out_b[0]) <= 1)
        cms.fetch_(ca, ma)
        cms.fetch_(cb, mb)
        worst = 0.0
        for c in range(nch):
            sa, sb = snapshot(ca.chains[c]), snapshot(cb.chains[c])
            assert sa.keys() == sb.keys()
            for k in sa:
                big = np.abs(sb[k]).max()
                assert big > 0 or not sa[k].any(), k
                if big > 0:
                    worst = max(worst, np.abs(sa[k] - sb[k]).max() / big)
                    assert np.abs(sa[k] - sb[k]).max() <= 1e-8 * big, (c, k)
        print("make_measurements_: device-drawn against the explicit batch, worst %.2e of an array's largest element (bound 1e-8)" % worst)
    finally:
        ma.close()
        mb.close()


# ---------------------------------------------------------------------------------------------- 5. states

def test_refusals_leave_the_handle_usable():
    from elphdynamics_amd import greens
    from elphdynamics_amd._lib import ELPH_E_ARG, ELPH_E_STATE
    m = make("b", 2, tol=1e-5)
    lib, h = m._lib, m._h
    try:
        n = C.c_uint64()
        assert lib.elph_greens_set_rng(h, 5) == ELPH_E_STATE and lib.elph_greens_rng_batches(h, C.byref(n)) == ELPH_E_STATE     # no estimator yet
        assert lib.elph_greens_update_rng(h, 0, None, None, None) == ELPH_E_STATE
        est = greens.EstimateGreensFunction(m, nv=3)
        assert lib.elph_greens_update_rng(h, 0, None, None, None) == ELPH_E_STATE                   # an estimator, but no generator
        assert b"elph_greens_set_rng" in lib.elph_last_error()
        est.device_rng_(5)
        assert lib.elph_greens_update_rng(h, 0, None, None, None) == ELPH_E_ARG                     # 3 vectors for 2 resident chains
        assert b"2 chains" in lib.elph_last_error() and batches_of(m) == 0                          # ... and no batch was drawn
        assert lib.elph_greens_update(h, None, 0, None, None, None) == ELPH_E_ARG                   # R = NULL is still refused there
        est = greens.EstimateGreensFunction(m, nv=4)                                                # a new estimator: the generator is gone
        assert not est.device_rng
        assert lib.elph_greens_update_rng(h, 0, None, None, None) == ELPH_E_STATE
        est.device_rng_(5)
        it, res, fl = greens.update_(est, m)                                                        # and the handle works
        assert not fl.any() and batches_of(m) == 1
        assert np.allclose(fetch_R(m, 4), batch(5, 1, 4, m.Ndim), rtol=0, atol=1e-12)
        rng = np.random.default_rng(3)                                                              # an explicit R wins, and draws nothing
        R = rng.standard_normal((4, m.Ndim))
        greens.update_(est, m, R=R)
        assert batches_of(m) == 1 and np.array_equal(est.R, R) and np.allclose(fetch_R(m, 4), R, rtol=0, atol=0)
    finally:
        m.close()


def test_the_two_generators_count_their_batches_apart():
    from elphdynamics_amd import greens, hmc, preconditioners as pc
    m = make("b", tol=1e-7)
    try:
        fa = pc.FourierAccelerator(m)
        pc.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
        H = hmc.HybridMonteCarlo(m, fa, dt=0.05, tr=0.1, alpha=0.1, Nb=1)
        H.device_rng_(11)
        est = greens.EstimateGreensFunction(m, nv=2)
        est.device_rng_(12)

        def hmc_batches():
            n = C.c_uint64()
            assert m._lib.elph_hmc_rng_batches(m._h, C.byref(n)) == 0
            return n.value

        hmc.update_(m, H, fa, None)
        nh = hmc_batches()
        assert nh > 0 and batches_of(m) == 0
        greens.update_(est, m)
        greens.update_(est, m)
        assert hmc_batches() == nh and batches_of(m) == 2
        assert np.allclose(fetch_R(m, 2), batch(12, 2, 2, m.Ndim), rtol=0, atol=1e-12)
        hmc.update_(m, H, fa, None)
        assert hmc_batches() == 2 * nh and batches_of(m) == 2
    finally:
        m.close()
