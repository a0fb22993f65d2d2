"""Device time of the chain diagnostics (gpt_amd/csrc/diag.hip) at four store shapes (P, T, M) and
lags K, written to profiles/diag_bench.json:

    PowerPlantNoTensor epoch ends   (2000, 100, 8),    K = 99
    every step kept                 (2000, 10000, 8),  K = 256
    w of a tensor sweep, small P    (200, 10000, 64),  K = 256
    kin40k predictions              (30000, 224, 8),   K = 223

Per shape: the evaluator's device-event time on a device store (gpt_diag_last_timing: the mean, the
autocovariance and the finishing kernels; median, min and max of --reps calls), its GB/s on two
reads of the window, its fp64 multiply-add rate as a share of the fp64 VALU peak (78.6 TFLOP/s,
half the fp32 vector peak), the numpy restatement (tests/diag_ref.py) with the rows split over 16
threads, and, for the autocovariance part alone, torch.fft.rfft -> |.|^2 -> irfft of the centred
store on the same device (event-timed, the centring left out).

    python scripts/time_diag.py [--reps 7] [--no-numpy] [--headline-ab FILE]

--headline-ab merges a json of alternating bench.py results of this library and the parent commit's
(GPTSGLD_LIB) into the output as `headline_ab`; an existing one is kept otherwise."""
import argparse
import concurrent.futures
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = {"powerplant_epoch_ends": (2000, 100, 8, 99), "every_step_kept": (2000, 10000, 8, 256),
          "tensor_sweep_w_small_P": (200, 10000, 64, 256), "kin40k_predictions": (30000, 224, 8, 223)}
FP64_VALU_PEAK = 78.6e12            # FLOP/s


def numpy_16_threads(x, K):
    import diag_ref as DR
    P, T, M = x.shape
    cuts = np.linspace(0, P, 17).astype(int)
    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda k: DR.diag_np(x[cuts[k]:cuts[k + 1]], 0, T, K), range(16)))
    return 1e3 * (time.perf_counter() - t0)


def fft_acov_ms(xt, K, reps):
    """rfft -> |.|^2 -> irfft along the samples of the centred (M, T, P) store, lags 0..K kept."""
    import torch
    M, T, P = xt.shape
    nfft = 1 << (T + K).bit_length()
    c = xt - xt.mean(dim=1, keepdim=True)
    ms = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f = torch.fft.rfft(c, n=nfft, dim=1)
        acov = torch.fft.irfft(f.real ** 2 + f.imag ** 2, n=nfft, dim=1)[:, :K + 1] / T
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
        del f
    return statistics.median(ms[1:]), acov


def one_shape(name, shape, reps, with_numpy):
    import torch
    from gpt_amd import GPT_SGLD as G
    from gpt_amd.session import diagnostics_device
    P, T, M, K = shape
    g = torch.Generator(device="cuda").manual_seed(5)
    e = torch.randn((M, T, P), dtype=torch.float64, device="cuda", generator=g)
    xt = torch.empty_like(e)                         # AR(1), phi = 0.5, unit variance
    xt[:, 0] = e[:, 0]
    for t in range(1, T):
        xt[:, t] = 0.5 * xt[:, t - 1] + 0.75 ** 0.5 * e[:, t]
    del e
    dev = []
    for _ in range(reps + 1):                        # the first call carries the module load
        d = diagnostics_device(xt, max_lag=K, acf=True)
        dev.append(G.diag_last_timing())
    ms = statistics.median(dev[1:])
    fma = P * M * sum(T - k for k in range(K + 1))
    fft_ms, acov = fft_acov_ms(xt, K, reps)
    out = dict(P=P, T=T, M=M, K=K, device_ms=ms, device_ms_min=min(dev[1:]), device_ms_max=max(dev[1:]),
               gbps_two_reads=2 * 8e-6 * P * T * M / ms, fma_per_s=fma / (ms * 1e-3),
               share_of_fp64_valu_peak=2 * fma / (ms * 1e-3) / FP64_VALU_PEAK,
               torch_fft_acov_ms=fft_ms, max_rhat=d.max_rhat, min_ess=d.min_ess,
               n_truncated=d.n_truncated)
    del acov
    if with_numpy:
        x = xt.cpu().numpy().transpose(2, 1, 0)     # (P, T, M), column-major
        out["numpy_16_threads_ms"] = numpy_16_threads(x, K)
        out["faster_than_numpy"] = ms < out["numpy_16_threads_ms"]
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--headline-ab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_bench.json"))
    args = ap.parse_args()
    old = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out = {"shapes": {k: one_shape(k, s, args.reps, not args.no_numpy) for k, s in SHAPES.items()}}
    if args.headline_ab:
        out["headline_ab"] = json.load(open(args.headline_ab))
    elif "headline_ab" in old:
        out["headline_ab"] = old["headline_ab"]
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
