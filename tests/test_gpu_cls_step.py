"""The full-theta softmax sampler on the device (ntc_chain_kernel, gpt_amd/csrc/cls.hip) against
mpmath at rounding level, at every class width and LDS edge of the kernel.

Every case of tests/cls_step_cases.py runs through GPT_SGLD.GPNT_SGLDclass_chains (one chain, `ncls`
given, the case's store_every); every stored step is held to the 50-digit reference of
tests/golden/cls_step_mp.npz within B·max|theta| of that step.  The reference draws its step noise by
Box–Muller in mpmath on the Philox integers, so no allowance for the device's normals is added.
What each case reaches (tests/test_cls_step_cases.py asserts it from a restatement of ntc_layout):

    cc32_min          C = 17: the smallest C of ntc_chain_kernel<32>; n = 70; last batch of 3; eps = 0.5
    cc32_full         C = 32: lanes 0..31 write P; n = 33 < 64; also through GPNT_SGLDclass
    one_class         C = 1 on the CC = 2 build, P ≡ 0; also through GPNT_SGLDclass
    absent_classes    labels {2, 3} with ncls = 5: three columns see prior and noise and +P·phi only
    stage_last        n = 307, m = 64: 163 664 B of LDS, the largest n that stages the batch
    stage_first_off   n = 308: the batch is re-read from HBM
    theta_fills_lds   n = 630, C = 32: theta alone is 161 280 B; n = 640 is refused before any launch
    saturated         sigma_theta = 500: max|x| > 800 at step 1, P is 0 or 1 to the last bit
    wide_batch        one batch of 96 columns over 8 waves, CC = 8, decay 0.5
    two_launches      4097 steps in the epoch: launches of 4096 and 1; every 241st step kept, the last
                      one computed by the second launch; a sibling chain equals its own run
    store_tail        10 steps, store_every = 4: 2 kept, the tail unsaved
    old_*             the six cases of tests/test_gpu_cls.py::test_sampler_matches_the_restatement

B = 8·u per case, u the error of the numpy restatement cls_ref.gpnt_sgld_class against the same
reference (tests/golden/make_cls_step_golden.py measures it: 8 s on eight processes;
tests/test_cls_step_cases.py holds B <= 1e-14 up to ten steps and <= 1e-13 always, and shows that
five defects of 1e-9 and below fail B).  The margin of 8 is tests/test_gpu_step.py's: other summation
orders (the wave sums of the n-long dot, the fma chain over the batch), the device library's exp, log
and pow, and theta0 and the noise drawn by the library's own Box–Muller.

Measured (u by the maker; device error / B as this file prints it, MI355X):
    case                         u         B = 8·u   device error / B
    cc32_min                     4.59e-16  3.67e-15  0.054
    cc32_full                    2.68e-16  2.14e-15  0.116
    one_class                    1.60e-16  1.28e-15  0.125
    absent_classes               1.14e-16  9.12e-16  0.125
    stage_last                   1.38e-16  1.10e-15  0.125
    stage_first_off              1.37e-16  1.10e-15  0.125
    theta_fills_lds              1.56e-16  1.25e-15  0.109
    saturated                    2.72e-16  2.18e-15  0.125
    wide_batch                   1.12e-16  8.98e-16  0.125
    two_launches                 2.70e-15  2.16e-14  0.112
    store_tail                   2.37e-16  1.90e-15  0.125
    old_70_130_3_25_1_2_0.1_1    3.78e-16  3.02e-15  0.125
    old_150_203_7_50_0_2_0_1     3.87e-16  3.09e-15  0.125
    old_64_96_2_96_0_3_0.5_0.7   1.24e-16  9.91e-16  0.125
    old_33_64_16_7_0_1_0_1       1.96e-16  1.57e-15  0.181
    old_20_10_2_50_0_2_0_1       7.38e-17  5.90e-16  0.240
    old_330_70_2_64_0_2_0_1      1.50e-16  1.20e-15  0.125
The single-entry runs and the two-chain run give their cases' figures again.  Where the ratio is
0.125 the device's worst element is the numpy restatement's, with the same double in it.  21 tests,
under 3 s on MI355X.
"""
import numpy as np
import pytest

import cls_step_cases as T

pytestmark = pytest.mark.gpu


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def run_chains(c, seeds=(T.SEED,), n=None):
    phi, y = T.inputs(c.name)
    if n is not None:
        phi = np.asfortranarray(np.resize(phi, (n, c.N)))
    return G().GPNT_SGLDclass_chains(phi, y, c.sigma, c.m, [c.eps] * len(seeds), c.decay, 0, c.epochs,
                                     list(seeds), store_every=c.store_every, ncls=c.C)


def hold(c, store):
    """Shape, finiteness and every stored step within B; prints device error / B."""
    ref = T.reference(c.name)
    assert store.shape == (c.n, c.C, T.kept(c))
    assert np.isfinite(store).all()
    err = T.step_errors(store, ref)
    print("%-30s u %.2e  B %.2e  device error / B %.3f (%.2e)" % (c.name, ref["u"], ref["bar"],
                                                                 err.max() / ref["bar"], err.max()))
    assert (err <= ref["bar"]).all(), (c.name, err / ref["bar"])


@pytest.mark.parametrize("c", T.CASES, ids=[c.name for c in T.CASES])
def test_sampler_against_mpmath(c):
    store, status = run_chains(c)
    assert status.shape == (1,) and status[0] == 0 and store.shape[3] == 1
    hold(c, store[..., 0])


@pytest.mark.parametrize("name", ["one_class", "cc32_full"])
def test_single_entry_against_mpmath(name):
    """GPNT_SGLDclass finds C = max(y) − min(y) + 1 itself: 1 and 32."""
    c = T.BY_NAME[name]
    assert c.store_every == 1
    phi, y = T.inputs(name)
    hold(c, G().GPNT_SGLDclass(phi, y, c.sigma, c.m, c.eps, c.decay, 0, c.epochs, T.SEED))


def test_launch_boundary_is_per_chain():
    """Two chains across the 4096-step boundary in one call: theta goes to HBM and comes back per
    chain, so each equals its own single run bit for bit, and the first is the case itself."""
    c = T.BY_NAME["two_launches"]
    other = 2 ** 40 + 9
    store, status = run_chains(c, (T.SEED, other))
    assert not status.any() and store.shape == (c.n, c.C, T.kept(c), 2)
    hold(c, store[..., 0])
    for k, seed in enumerate((T.SEED, other)):
        alone, st = run_chains(c, (seed,))
        assert st[0] == 0 and np.array_equal(alone[..., 0], store[..., k]), k
    assert not np.array_equal(store[..., 0], store[..., 1])


def test_theta_past_lds_is_refused():
    """n = 640, C = 32: theta alone is 160 KiB; GPT_ERR_BAD_DIMS, nothing launched, nothing written."""
    from gpt_amd import _lib
    c = T.BY_NAME["theta_fills_lds"]
    with pytest.raises(_lib.GPTError) as e:
        run_chains(c, n=T.REFUSED_N)
    assert e.value.code == _lib.GPT_ERR_BAD_DIMS
    assert "160 KiB" in str(e.value)
