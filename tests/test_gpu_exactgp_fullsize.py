"""The reference's quality-ceiling row on the device: PowerPlant exact GP, 5000 train / 4568 test,
test RMSE 4.0056 (DataRecords.txt:19).

Split: the first 5000 rows of tests/golden/powerplant.npz whitened with their own mean and std,
the remaining 4568 rows shifted and scaled by the train statistics (this split gives the recorded
mean-prediction RMSE 17.1331).  Hyper-parameters: iso length_scale 1.4332, sigma_RBF 1,
signal_var 0.2299^2.  cond(A) is about 3e4: 3e4 x 1.1e-16 with a growth allowance of a few hundred
gives the 1e-9 bars of fmu, alpha and fs2 (test_theta_mean's bar); the value is held to 1e-10.
"""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
H = np.array([1.4332, 1.0, 0.2299 ** 2])
NTRAIN = 5000


def split():
    pp = np.load(os.path.join(HERE, "golden", "powerplant.npz"))["data"]
    Xa, ya = pp[:, :4], pp[:, 4]
    mu, sd = Xa[:NTRAIN].mean(axis=0), Xa[:NTRAIN].std(axis=0, ddof=1)
    ym, ys = ya[:NTRAIN].mean(), ya[:NTRAIN].std(ddof=1)
    Xw, yw = (Xa - mu) / sd, (ya - ym) / ys
    return Xw[:NTRAIN], yw[:NTRAIN], Xw[NTRAIN:], yw[NTRAIN:], ym, ys, ya[NTRAIN:]


def restatement(X, y, Xt, h):
    """scipy fp64: value, alpha, fmu, fs2"""
    from scipy.linalg import cho_solve, cholesky, solve_triangular
    from scipy.spatial.distance import cdist
    ls, sigma, s2 = h
    K = sigma ** 2 * np.exp(-0.5 * cdist(X / ls, X / ls, "sqeuclidean"))
    K[np.diag_indices_from(K)] += s2
    L = cholesky(K, lower=True, overwrite_a=True, check_finite=False)
    alpha = cho_solve((L, True), y, check_finite=False)
    val = np.log(np.diag(L)).sum() + 0.5 * (y @ alpha) + 0.5 * y.size * math.log(2 * math.pi)
    Ks = sigma ** 2 * np.exp(-0.5 * cdist(X / ls, Xt / ls, "sqeuclidean"))
    fmu = Ks.T @ alpha
    V = solve_triangular(L, Ks, lower=True, overwrite_b=True, check_finite=False)
    fs2 = np.maximum(sigma ** 2 - np.einsum("ij,ij->j", V, V), 0.0)
    return val, alpha, fmu, fs2


def test_powerplant_quality_ceiling():
    pytest.importorskip("scipy")
    from gpt_amd import GPT_SGLD as G
    X, y, Xt, yt, ym, ys, yraw = split()
    assert Xt.shape[0] == 4568
    assert abs(math.sqrt(np.mean((yraw - ym) ** 2)) - 17.1331) <= 1e-4      # the recorded split (17.13318)
    gp = G.ExactGP(X, y)
    val = gp.nlogmarginal(H)
    alpha = gp.alpha(H)
    pr = gp.predict(H, Xt, yt)
    rv, ra, rmu, rs2 = restatement(X, y, Xt, H)
    rmse = ys * math.sqrt(np.mean((yt - pr.fmu) ** 2))
    e_val = abs(val - rv) / abs(rv)
    e_mu = np.abs(pr.fmu - rmu).max() / np.abs(rmu).max()
    e_al = np.abs(alpha - ra).max() / np.abs(ra).max()
    e_s2 = np.abs(pr.fs2 - rs2).max() / H[1] ** 2
    print("N = 5000: nlml %.6f (restatement %.6f), value %.2e, fmu %.2e, alpha %.2e, fs2 %.2e, "
          "ytrainStd x RMSE %.4f (restatement %.4f)"
          % (val, rv, e_val, e_mu, e_al, e_s2, rmse, ys * math.sqrt(np.mean((yt - rmu) ** 2))))
    assert e_val <= 1e-10
    assert e_mu <= 1e-9 and e_al <= 1e-9
    assert e_s2 <= 1e-9
    assert abs(rmse - 4.0056) <= 5e-4
    assert np.array_equal(pr.ys2, pr.fs2 + H[2]) and np.isfinite(pr.lp).all()
