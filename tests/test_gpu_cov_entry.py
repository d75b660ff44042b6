"""What csrc/cov_entry.h guarantees, at EVERY unrolled feature count: a covariance entry has the same bits wherever it is
computed.  N = 67 is odd (the odd tail of the two-observation loop of kstar_mu_kernel) and one slice of 64 observations plus
three; M = 1030 leaves the last thread of the pair kernels with one real and one missing candidate, off the chunk granule;
chunk = 512 cuts the candidates into three chunks.  Every comparison is array_equal: there is no tolerance to work out."""
import numpy as np
import pytest

from bayesian_optimisation_amd import DeviceGP
from bayesian_optimisation_amd.synthetic import make_problem

pytestmark = pytest.mark.gpu

N, M, CHUNK = 67, 1030, 512


@pytest.mark.parametrize("d", range(1, 17))
def test_mean_is_the_fp64_routes_in_every_screen(d):
    """score_f32 (kstar_mu_kernel, float store), score_i8 and score_i8c (kstar_slices_kernel) against score (kstar_mu_kernel).
    A screen that falls back returns the fp64 pass's own mean, which would make the comparison vacuous: refused."""
    X, y, Xs, ls = make_problem(N, M, d)
    gp = DeviceGP(chunk=CHUNK).factorise(X, y, ls)
    mu64 = gp.score(Xs, dense=True).mu.cpu().numpy()
    assert mu64.shape == (M,) and np.isfinite(mu64).all()
    for name in ("score_f32", "score_i8", "score_i8c"):
        mu = getattr(gp, name)(Xs, dense=True).mu.cpu().numpy()
        assert not gp.last_screen["fallback"], (name, d, gp.last_screen)
        assert np.array_equal(mu, mu64), (name, d)


@pytest.mark.parametrize("d", range(1, 17))
def test_appended_column_of_k_is_the_factorisations(d):
    """append_kvec_kernel against kxx_kernel: K after N - 1 observations and one append() is K of N observations."""
    X, y, _, ls = make_problem(N, M, d)
    gp = DeviceGP(chunk=CHUNK).factorise(X[:N - 1], y[:N - 1], ls)
    gp.append(X[N - 1], y[N - 1])
    ref = DeviceGP(chunk=CHUNK).factorise(X, y, ls)
    assert gp.N == N
    assert np.array_equal(gp.K[:N, :N].cpu().numpy(), ref.K[:N, :N].cpu().numpy())


@pytest.mark.parametrize("family", ["matern32", "matern52"])
@pytest.mark.parametrize("d", [1, 5, 16])
def test_matern_tail_and_pair_paths_agree(family, d):
    """Chunks of 512 and of 1024 give the same mean: the Matern instances of the odd tail, of the two-observation loop and of
    the half-empty last thread (M = 1030 = 2 x 512 + 6 = 1024 + 6) use one entry formula."""
    X, y, Xs, ls = make_problem(N, M, d)
    a = DeviceGP(chunk=512).factorise(X, y, ls, kernel=family).score(Xs, dense=True).mu.cpu().numpy()
    b = DeviceGP(chunk=1024).factorise(X, y, ls, kernel=family).score(Xs, dense=True).mu.cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a, b)
