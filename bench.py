#!/usr/bin/env python3
"""bench.py — GP fit+predict throughput of the MI355X engine on BASELINE.json's metric configuration.

One "step" = one fixed-work fit + one batched predict on config M (rosenbrock d=8, n=4096, f64):
  * fit: (1 + R) = 3 bounded L-BFGS runs x 150 log-marginal-likelihood+gradient evaluations (the reference's cap:
    gpr.rs:222 n_restarts_optimizer = 2, gradmin.rs:54 maxeval = 150), K^-1 of the captured best evaluation,
  * predict: mean + variance at m = 1600 candidates (about one generation of the caller's predict calls).
Inputs are synthetic (hbetune_rs_amd/synth.py), uploaded to HBM inside the C ABI call; the timed region covers the
whole fit+predict call chain (H2D of X, y is ~300 KB and included).

Multi-GPU (`--gpus N`): the path shards as independent units with no exchange step: every rank runs
whole fit+predict steps on its own GPU ("weak" scaling, no data-path collective); torch.distributed (RCCL) is only used
for the barrier and the max-over-ranks of the timings.  Started without a torchrun environment, `--gpus N` launches its
own N ranks (`python -m torch.distributed.run ... bench.py`) before anything touches a GPU and relays their output.

`--workload C3` is BASELINE.json's sharded configuration (rastrigin d=16, n=4096, 1 + 7 optimiser runs,
gradmin.rs:19-31): ONE process owns `--gpus G` devices through hbegp_ctx_create(G), run r goes to device r mod G, the
host picks the arg-max ("strong" scaling: the 8 runs are the fixed total work).

A plain run sets up, warms up, times the steps, writes `--dump-outputs` and prints the headline line.  `--full` adds, after
the timed steps, everything else the bench measures or checks: the roofline (kernel timings in runs of their own), the CPU
baseline with the in-run parity check against the oracle and the referee, and the side lines (converged fit, f32, the other
BASELINE configurations, small n, concurrent fits); `--no-cpu-baseline` and `--no-side-lines` trim a `--full` run.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP64_MFMA_TFLOPS = 78.6   # MI355X fp64 matrix peak (vendor); tools/ubench.hip measures 77.1
PEAK_FP32_MFMA_TFLOPS = 157.3  # fp32-input MFMA (= the fp32 vector rate)
PEAK_HBM_TBS = 8.0
N_CUS = 256
EVALS_PER_RUN = 150
N_RESTARTS = 2
M_CANDIDATES = 1600
REFEREE_M = 64      # candidates the extended-precision referee re-derives (parity_in_run.timed_model.referee)


_T0 = time.time()


def log(msg):
    """Progress on stderr (stdout carries the one JSON line): a silent multi-minute run looks hung to a driver."""
    print(f"[bench {time.time() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(w, theta, Xs, n_evals, reps=5, parity=None):
    """The reference's CPU path restated, timed on this box's host cores in the same run.  Main line (`value`):
    oracle/gpr_oracle.py -- the reference-faithful algorithm incl. the materialised dK tensor and LAPACK potrf/potrs/potri -- on
    ONE thread (the reference builds OpenBLAS with USE_THREAD=0, Makefile:3-4): median of `reps` full-size lml+gradient
    evaluations + one predict; the fit's evaluations are extrapolated from that median (a bounded sample: ~30 s of CPU work).
    Beside it: the same port on all cores (best effort), the LAPACK-free C restatement oracle/gpr_oracle.c on a reduced-n sample,
    dpotrf+dpotri alone on all cores (a floor for any CPU implementation) and torch's Cholesky + inverse as a cross-check."""
    import numpy as np
    from threadpoolctl import threadpool_limits

    from oracle import gpr_oracle as O

    n = w["n"]
    s2, c, ell = math.exp(theta[0]), math.exp(theta[1]), np.exp(theta[2:])
    ncores = os.cpu_count()
    t_evals = []
    log(f"cpu baseline: {reps} full-size evaluations of the numpy/LAPACK port on 1 thread")
    with threadpool_limits(limits=1):
        for _ in range(reps):
            t0 = time.perf_counter()
            res = O.lml_with_gradient(w["X"], w["y"], s2, c, ell, 2.5)
            t_evals.append(time.perf_counter() - t0)
            log(f"  evaluation {len(t_evals)}: {t_evals[-1]:.2f} s")
        t0 = time.perf_counter()
        O.predict(Xs, w["X"], res["alpha"], res["k_inv"], c, ell, 2.5)
        t_pred = time.perf_counter() - t0
    if parity is not None:
        parity(O, res)  # the checker's results are in hand: put the GPU's next to them (never inside a timed region)
    t_eval = sorted(t_evals)[len(t_evals) // 2]
    fit_predict_s = n_evals * t_eval + t_pred
    out = {
        "value": 1.0 / fit_predict_s,
        "unit": "fit+predict/s",
        "cores": 1,
        "kind": "port",
        "sample": f"extrapolated x{n_evals} from the median of {reps} full-size lml+gradient evaluations ({t_eval:.2f} s each: "
                  f"{', '.join(f'{t:.2f}' for t in t_evals)}) + 1 predict m={len(Xs)} ({t_pred:.2f} s), n={n} d={w['d']} f64, "
                  f"oracle/gpr_oracle.py (numpy + LAPACK dpotrf/dpotrs/dpotri, materialised dK tensor), 1 thread",
        "eval_s": t_eval,
        "predict_s": t_pred,
        "nproc": ncores,
        "cpu_model": _cpu_model(),
    }
    # best effort: the same port with every host core (LAPACK threads; the tensor passes stay numpy's)
    log("cpu baseline: the same port on all cores")
    t0 = time.perf_counter()
    O.lml_with_gradient(w["X"], w["y"], s2, c, ell, 2.5)
    t_all = time.perf_counter() - t0
    out["best_effort_all_cores"] = {"cores": ncores, "eval_s": t_all, "value": 1.0 / (n_evals * t_all + t_pred),
                                    "sample": "1 full-size evaluation of the same port, all host cores"}
    # the floor of any CPU implementation on this box: LAPACK dpotrf + dpotri alone (n^3 flops), all cores
    from scipy.linalg import lapack

    Kc = res["kernel_matrix"].copy()
    log("cpu baseline: LAPACK dpotrf + dpotri, all cores")
    t0 = time.perf_counter()
    ch, _ = lapack.dpotrf(Kc, lower=1)
    lapack.dpotri(ch, lower=1)
    t_lapack_all = time.perf_counter() - t0
    out["floor_all_cores"] = {"cores": ncores, "lapack_only_eval_s": t_lapack_all, "value": 1.0 / (n_evals * t_lapack_all + t_pred),
                              "note": "dpotrf + dpotri alone on all host cores: a floor for any CPU implementation of one evaluation"}
    # the LAPACK-free plain-C restatement (oracle/gpr_oracle.c), 1 thread: far too slow for a full-size sample (unblocked loops,
    # ~150 s per evaluation at n=4096), so a reduced-n sample scaled by (n / n_sample)^3 -- a LOWER bound on its full-size time
    try:
        from hbetune_rs_amd import synth
        from oracle import c_oracle as CO

        ns = 1024
        log("cpu baseline: plain-C restatement, n=1024 sample x3")
        ws = synth.make_workload("M", n=ns)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            CO.lml_with_gradient(ws["X"], ws["y"], s2, c, np.exp(ws["theta"][2:]), 2.5)
            ts.append(time.perf_counter() - t0)
        t_c = sorted(ts)[1]
        out["c_port_scaled_sample"] = {"cores": 1, "kind": "port", "eval_s_at_sample": t_c, "n_sample": ns,
                                       "eval_s_scaled": t_c * (n / ns) ** 3, "value": 1.0 / (n_evals * t_c * (n / ns) ** 3 + t_pred),
                                       "sample": f"median of 3 evaluations of oracle/gpr_oracle.c at n={ns} (config M data), scaled by ({n}/{ns})^3"}
    except Exception as e:  # the C oracle is test infrastructure: its absence must not cost the bench line
        out["c_port_scaled_sample"] = {"error": str(e)}
    # optimised-LAPACK cross-check through torch (CPU): Cholesky + inverse only
    try:
        import torch

        Kt = torch.from_numpy(res["kernel_matrix"].copy())
        tt = {}
        many = min(ncores, 16)  # torch.cholesky_inverse with 256 threads took 389 s on the GPU box's EPYC 9575F (1.7 s on one)
        for nthreads in (1, many):
            log(f"cpu baseline: torch cholesky + cholesky_inverse, {nthreads} thread(s)")
            torch.set_num_threads(nthreads)
            t0 = time.perf_counter()
            L = torch.linalg.cholesky(Kt)
            torch.cholesky_inverse(L)
            tt[nthreads] = time.perf_counter() - t0
        out["torch_cholesky_plus_inverse_s"] = {"1_thread": tt[1], f"{many}_threads": tt[many]}
    except Exception as e:
        out["torch_cholesky_plus_inverse_s"] = {"error": str(e)}
    return out


PARITY_BAR = 1e-8  # north_star: f64 results within 1e-8 of the reference's CPU path


def parity_in_run(gpr, ctx, w, theta, Xs, timed_model, O, ref):
    """The oracle (the CHECKER -- the reference's lml.rs:29-79 / predict.rs:7-52 restated, oracle/gpr_oracle.py) next to the GPU at
    the headline size, in the run that produced the number: (a) one lml+gradient evaluation and a model built at the bench's theta
    against the oracle's evaluation at that theta (already computed by the cpu_baseline leg); (b) the TIMED model (the last
    fixed-work fit of the timed region) against one more oracle evaluation at the theta that fit captured.  Deviations are
    relative to max(1, scale) as in tests/test_gpu_parity.py; the variance is relative to the amplitude."""
    import numpy as np

    X, y = w["X"], w["y"]
    s2, c, ell = math.exp(theta[0]), math.exp(theta[1]), np.exp(theta[2:])
    prob = gpr.Problem(X, y, nu=2.5, ctx=ctx)
    lml, grad = prob.lml_with_gradient(theta)
    alpha, kinv, _ = prob.results()
    prob.close()
    fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5, ctx=ctx)
    mean, var, _ = fk.predict(Xs)
    fk.release()
    rm, rv, _ = O.predict(Xs, X, ref["alpha"], ref["k_inv"], c, ell, 2.5)
    rel = lambda got, want: float(np.max(np.abs(np.asarray(got) - np.asarray(want))) / max(1.0, float(np.max(np.abs(want)))))
    out = {
        "bar": PARITY_BAR,
        "lml_rel": abs(lml - ref["lml"]) / max(1.0, abs(ref["lml"])),
        "grad_rel": rel(grad, ref["grad"]),
        "alpha_rel": rel(alpha, ref["alpha"]),
        "kinv_rel": rel(np.tril(kinv), np.tril(ref["k_inv"])),
        "mean_abs": rel(mean, rm),
        "var_abs": float(np.max(np.abs(var - rv)) / c),
        "at": "the bench's theta (SURVEY 8d), n=%d d=%d, m=%d candidates" % (X.shape[0], X.shape[1], len(Xs)),
    }
    if timed_model is not None:
        tth = timed_model["theta"]
        s2t, ct, ellt = math.exp(tth[0]), math.exp(tth[1]), np.exp(tth[2:])
        log("parity: one more oracle evaluation at the timed fit's captured theta")
        rt = O.lml_with_gradient(X, y, s2t, ct, ellt, 2.5)
        rmt, rvt, _ = O.predict(Xs, X, rt["alpha"], rt["k_inv"], ct, ellt, 2.5)
        # The fit ends where the optimiser drove it (typically tiny noise: cond(K) ~ 1e11..1e12), and there a LAPACK solve is itself
        # good to ~cond(K) eps only.  So the extended-precision referee (oracle/referee.py: K in binary128, iterative refinement with
        # double-double residuals, double-double Cholesky for the log-determinant) supplies the truth, and the rule is
        #   |gpu - truth| <= max(1e-8 * scale, 2 * |lapack - truth|)
        # -- the engine may be at most twice as far from the truth as the reference's own arithmetic.  `ok_1e-8` keeps the plain
        # verdict against the oracle beside it.
        ev = np.linalg.eigvalsh(rt["kernel_matrix"])
        cond = float(ev[-1] / ev[0])
        tm_dev = {
            "lml_rel": abs(timed_model["lml"] - rt["lml"]) / max(1.0, abs(rt["lml"])),
            "mean_abs": rel(timed_model["mean"], rmt),
            "var_abs": float(np.max(np.abs(timed_model["var"] - rvt)) / ct),
        }
        tm = dict(tm_dev, cond_K=cond, ok_1e_8=bool(max(tm_dev.values()) <= PARITY_BAR),
                  at="the theta captured by the last timed fit; its predictions at the m candidates are the timed ones")
        tm["ok_1e-8"] = tm.pop("ok_1e_8")
        try:
            from oracle import referee as RF

            t0 = time.perf_counter()
            log("parity: the referee at the captured theta (binary128 kernel matrix, refined solves, double-double Cholesky)")
            rf = RF.Referee(X, y, s2t, ct, ellt, 2.5)
            mr = min(REFEREE_M, len(Xs))  # every candidate costs one refined solve with the n x n double-double matrix
            t_mean, t_var, _ = rf.predict(Xs[:mr])
            t_lml = rf.lml()
            ah, al = rf.alpha()
            t_alpha = ah + al
            rf.close()

            def three(got, lap, truth, scale):
                e_g, e_l = float(np.max(np.abs(np.asarray(got) - truth))) / scale, float(np.max(np.abs(np.asarray(lap) - truth))) / scale
                return {"gpu_vs_truth": e_g, "lapack_vs_truth": e_l, "allowed": max(PARITY_BAR, 2.0 * e_l), "ok": bool(e_g <= max(PARITY_BAR, 2.0 * e_l))}

            verdicts = {
                "lml": three([timed_model["lml"]], [rt["lml"]], np.array([t_lml]), max(1.0, abs(t_lml))),
                "mean": three(timed_model["mean"][:mr], rmt[:mr], t_mean, max(1.0, float(np.max(np.abs(t_mean))))),
                "var": three(timed_model["var"][:mr], rvt[:mr], t_var, ct),
            }
            if timed_model.get("alpha") is not None:
                verdicts["alpha"] = three(timed_model["alpha"], rt["alpha"], t_alpha, max(1.0, float(np.max(np.abs(t_alpha)))))
            tm["referee"] = dict(verdicts, m_candidates=mr, rule="|gpu - truth| <= max(1e-8, 2 |lapack - truth|), deviations relative to max(1, scale) (variance: to the amplitude)",
                                 refinement_sweeps=[len(h) for h in rf.sweeps], seconds=time.perf_counter() - t0)
            tm["ok"] = all(v["ok"] for v in verdicts.values())
        except Exception as e:  # the referee is test infrastructure: without it only the plain verdict stands
            tm["referee"] = {"error": repr(e)}
            tm["ok"] = tm["ok_1e-8"]
        out["timed_model"] = tm
    worst = max(v for k, v in out.items() if k.endswith(("_rel", "_abs")))
    out["worst"] = worst
    out["ok"] = bool(worst <= PARITY_BAR) and out.get("timed_model", {}).get("ok", True)
    return out


DUMP_LIMIT_BYTES = 64 << 20
KINV_SAMPLE = 1 << 20  # K^-1 entries kept by --dump-outputs (8 MB in f64; the full matrix is 128 MB at n = 4096)


def model_outputs(fk):
    """What a caller of FittedKernel.new receives, as float64 arrays: theta, lml, alpha and K^-1.  K^-1 is cut to a fixed
    sample of KINV_SAMPLE entries (row-major flat indices from a seeded generator, sorted) when it is larger than that; the
    indices are written beside it."""
    import numpy as np

    alpha, kinv = fk.arrays()
    out = {"theta": np.asarray(fk.theta, np.float64), "lml": np.array([fk.lml], np.float64), "alpha": alpha.astype(np.float64)}
    flat = kinv.astype(np.float64).ravel()
    if flat.size > KINV_SAMPLE:
        idx = np.sort(np.random.default_rng(20240917).choice(flat.size, KINV_SAMPLE, replace=False))
        out["kinv_sample"], out["kinv_sample_index"] = flat[idx], idx.astype(np.float64)
    else:
        out["kinv"] = kinv.astype(np.float64)
    return out


def dump_outputs(path, arrays):
    """--dump-outputs: one DIR/<name>.npy per array, float32 / float64 only, at most DUMP_LIMIT_BYTES in all."""
    import numpy as np

    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    for k, v in arrays.items():
        assert v.dtype in (np.float32, np.float64), (k, v.dtype)
    total = sum(v.nbytes for v in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit"
    os.makedirs(path, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(path, f"{k}.npy"), v)
    log(f"wrote {len(arrays)} arrays ({total / 1e6:.1f} MB) to {path}")


def self_launch(args):
    """`--gpus N` without a torchrun environment: start the N ranks ourselves (nothing in this process has touched a GPU),
    relay their output, return their exit code."""
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + [a for a in sys.argv[1:]]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["HBEGP_BENCH_CHILD"] = "1"
    return subprocess.call(cmd, env=env)


def kernel_table(tc, n, d, dtype_bytes=8):
    """Per-kernel-class roofline rows from hipEvent timings taken with every slot of a fit evaluating at once (the timed
    configuration).  `achieved` = algorithmic work of the class in ONE evaluation / the summed duration of its launches in
    that evaluation; `frac` is against the WHOLE chip's peak although the launch shares the chip with the other slots'
    launches; `share_of_round` = that duration / the wall time of a round in which every slot finishes one evaluation."""
    peak = PEAK_FP64_MFMA_TFLOPS if dtype_bytes == 8 else PEAK_FP32_MFMA_TFLOPS
    rnd = max(tc["round_eager_ms"], 1e-9)
    rows = []

    def mfma(name, ms, gflop, launches):
        if ms > 0:
            rows.append({"kernel": name, "bound": "mfma", "ms_per_eval": ms, "gflop_per_eval": gflop, "launches_per_eval": launches,
                         "achieved": gflop / ms, "unit": "TFLOP/s", "frac": gflop / ms / peak, "share_of_round": ms / rnd})

    def hbm(name, ms, mbytes):
        if ms > 0:
            rows.append({"kernel": name, "bound": "hbm", "ms_per_eval": ms, "mbytes_per_eval": mbytes, "launches_per_eval": 1,
                         "achieved": mbytes * 1e-6 / (ms * 1e-3), "unit": "TB/s", "frac": mbytes * 1e-6 / (ms * 1e-3) / PEAK_HBM_TBS,
                         "share_of_round": ms / rnd})

    wg = int(tc["task_queue_workgroups"])
    in_queue = wg and tc["lauum_ms"] <= 0  # the K^-1 = X^T X tiles are tasks of the same launch (the default)
    mfma(("dag_kernel (Cholesky + inverse factor + K^-1: diagonal blocks + tile tasks)" if in_queue else
          "dag_kernel (Cholesky + inverse factor: diagonal blocks + tile tasks)") if wg else
         "leaf_kernel + gemm_kernel launches (Cholesky + inverse factor)",
         tc["factor_ms"], tc["factor_gflop"], tc["factor_launches"])
    mfma("gemm_kernel (LAUUM: K^-1 = X^T X)", tc["lauum_ms"], tc["lauum_gflop"], 1)
    tri = n * n / 2 * dtype_bytes * 1e-6
    hbm("kmat_kernel (writes the lower triangle of K)", tc["kmat_ms"], tri + n * d * dtype_bytes * 1e-6)
    hbm("gradtrace_kernel (reads the lower triangle of K^-1)", tc["gradtrace_ms"], tri + n * (d + 1) * dtype_bytes * 1e-6)
    hbm("trmv/alpha kernels (read X = L^-1 twice)", tc["alpha_ms"], 2 * tri)
    return rows


def roofline_block(gpr, ctx, X, y, theta, nslots, ms_per_step, n_evals, extra_flop, pmc_ok=True, n_devices=1):
    """The roofline object of the bench line.  Kernel times come from the timed configuration: all `nslots` evaluation slots of a
    fit running at once on device 0, one hipEvent pair per launch group on each slot's stream (hbegp_problem_time_concurrent);
    the dominant class is chosen by its measured share.
      achieved = the co-resident launches together: nslots x (algorithmic GFLOP of ONE launch / its average duration) -- they
                 share the chip for their whole life, so their sum is what the chip delivers while they are in flight;
      peak     = the WHOLE chip's fp64 MFMA peak;   frac = achieved / peak.
    The per-launch figures (one launch against the whole chip, against the CUs it is sized for, against a 1/nslots share) are in
    `per_launch`; `whole_fit_frac_of_peak` is every flop of the step over the driver-visible wall time."""
    n, d = X.shape
    prob3 = gpr.Problem(X, y, nu=2.5, n_slots=nslots, ctx=ctx)
    tc = prob3.time_concurrent(theta, reps=5)
    prob3.close()
    kernels = kernel_table(tc, n, d)
    dom = max(kernels, key=lambda r: r["ms_per_eval"])
    wg = int(tc["task_queue_workgroups"])
    launches = max(dom.get("launches_per_eval", 1), 1)
    one = dom["achieved"]
    is_dag = bool(wg) and dom["kernel"].startswith("dag_kernel")
    co = nslots if is_dag else 1  # launches of this class in flight side by side
    peak = PEAK_FP64_MFMA_TFLOPS if dom["bound"] == "mfma" else PEAK_HBM_TBS
    traffic, traffic_note = None, None
    if pmc_ok and is_dag:
        try:
            src = next(f for f in ("r05_pmc_3slot.json", "r04_pmc_3slot.json", "r03_pmc_3slot.json") if os.path.exists(os.path.join(ROOT, "profiles", f)))
            pmc = json.load(open(os.path.join(ROOT, "profiles", src)))
            pmc = pmc.get("kernels", pmc)
            key = [k for k in pmc if "dag_kernel" in k]
            rec = pmc[key[0]]
            traffic = (rec.get("fetch_bytes_per_launch") or rec["fetch_bytes_per_dispatch"]) + (rec.get("write_bytes_per_launch") or rec["write_bytes_per_dispatch"])
            traffic_note = (f"FETCH_SIZE x2 + WRITE_SIZE per launch from profiles/{src}: ONE 96-workgroup launch running alone -- "
                            "rocprofv3 --pmc serialises dispatches, so counters of three co-resident launches cannot be collected; "
                            "algorithmic (compulsory) bytes per launch: K lower in, L / L^-1 / K^-1 lower out = 4 x n^2/2 x 8 B")
        except Exception:
            traffic = None
    prob1 = gpr.Problem(X, y, nu=2.5, ctx=ctx)
    ph = prob1.time_eval(theta, reps=5)
    prob1.close()
    return {
        "bound": dom["bound"],
        "kernel": dom["kernel"],
        "achieved": co * one,
        "peak": peak,
        "unit": dom["unit"],
        "frac": co * one / peak,
        "traffic": traffic,
        "traffic_config": traffic_note,
        "algorithmic_bytes_per_launch": 4 * n * n / 2 * 8 if is_dag else None,
        "note": (f"{co} task-queue launches ({wg} workgroups of 512 threads each, one per CU) are co-resident for their whole life, one per "
                 f"optimiser run: achieved = {co} x (68.72-GFLOP-class launch / its average duration), against the whole chip's peak. "
                 f"per_launch holds the single-launch readings.") if is_dag else "whole-chip launch",
        "per_launch": {"achieved": one, "frac_of_whole_chip": one / peak,
                       "frac_of_the_CUs_it_is_sized_for": (one / (peak * wg / N_CUS)) if is_dag else None,
                       "frac_of_a_1_over_nslots_share": one / (peak / co), "workgroups": wg},
        "launches_per_eval": launches,
        "gflop_per_launch": dom.get("gflop_per_eval", 0.0) / launches,
        "avg_launch_ms": dom["ms_per_eval"] / launches,
        "measured": f"hipEvents on each slot's stream, {nslots} slots evaluating at once, eager launches (hbegp_problem_time_concurrent)",
        "concurrent_round_ms": tc["round_ms"],
        "concurrent_round_eager_ms": tc["round_eager_ms"],
        "amortised_eval_ms_in_fit": ms_per_step / max(n_evals, 1),
        "single_stream_eval_ms": ph["eval_graph_ms"],
        "whole_eval_frac_of_peak": (n ** 3) * 1e-12 / (ph["eval_graph_ms"] * 1e-3) / PEAK_FP64_MFMA_TFLOPS,
        "whole_fit_frac_of_peak": (n_evals * n ** 3 + extra_flop) * 1e-12 / (ms_per_step * 1e-3) / (PEAK_FP64_MFMA_TFLOPS * n_devices),
        "kernels": [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()} for r in kernels],
        "single_stream_phases_ms": {k: round(v, 4) for k, v in ph.items()},
    }


def run_c3(args):
    """BASELINE.json configs[2]: rastrigin d=16, n=4096, f64, 8 optimiser runs sharded over G devices of ONE process."""
    import numpy as np  # noqa: F401
    import torch  # noqa: F401

    from hbetune_rs_amd import gpr, synth

    G = args.gpus
    w = synth.make_workload("C3", n=args.n)
    X, y = w["X"], w["y"]
    starts = synth.restart_points("C3", w["lo"], w["hi"], 7)
    ctx = gpr.Context(device_ids=list(range(G)))

    kept = []

    def step(keep=False):
        fk = gpr.FittedKernel.new(X, y, w["theta0"], w["lo"], w["hi"], starts, nu=2.5, ctx=ctx, maxeval=EVALS_PER_RUN, fixed_work=True)
        out = (fk.lml, fk.n_evals, fk.n_not_pd)
        if keep:
            kept.append(fk)  # --dump-outputs: the last timed fit is read back and released after the timed region
        else:
            fk.release()
        return out

    for _ in range(args.warmup):
        step()
    t0 = time.perf_counter()
    for i in range(args.steps):
        lml, n_evals, n_not_pd = step(keep=bool(args.dump_outputs) and i == args.steps - 1)
    elapsed = time.perf_counter() - t0
    if kept:
        dump_outputs(args.dump_outputs, model_outputs(kept[0]))
        kept[0].release()
    n, d = X.shape
    out = {
        "metric": "GP fits/sec (C3: rastrigin d=16, n=4096, f64, 8 optimiser runs sharded over the GPUs of one process)",
        "value": args.steps / elapsed, "unit": "fits/s", "n_gpus": G, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"C3: rastrigin d={d} n={n} f64, 1+7 L-BFGS runs x {EVALS_PER_RUN} evaluations, run r -> device r mod {G} "
                               f"(hbegp_ctx_create({G})), host arg-max over the captures, no collective",
                   "evals_per_fit": n_evals, "n_not_pd": n_not_pd, "parallelism": f"restarts x{G} in one process"},
        "fit_frac_of_peak": n_evals * n ** 3 * 1e-12 / (elapsed / args.steps) / (PEAK_FP64_MFMA_TFLOPS * G),
        "lml": lml,
    }
    if args.full:
        # the kernel the runs spend their time in, on device 0 with the slots one device runs side by side (8 runs over G
        # devices, at most 3 at once per device)
        nslots = max(1, min(3, -(-8 // G)))
        ctx0 = gpr.Context(device_ids=[0])
        out["roofline"] = roofline_block(gpr, ctx0, X, y, w["theta"], nslots, elapsed / args.steps * 1e3, n_evals, 0.0, pmc_ok=False, n_devices=G)
        ctx0.close()
    if args.full and not args.no_cpu_baseline:
        cb = cpu_baseline(w, w["theta"], synth.candidates("C3", 8, d), n_evals, reps=3)
        cb["value"] = 1.0 / (n_evals * cb["eval_s"])  # fits/s: no predict in this workload
        cb["unit"] = "fits/s"
        out["cpu_baseline"] = cb
        out["speedup_vs_cpu_port"] = out["value"] / cb["value"]
    print(json.dumps(out), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="M", choices=["M", "C3"])
    ap.add_argument("--n", type=int, default=None, help="override n (debug only; invalidates the metric)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything beyond the headline: roofline, CPU baseline "
                         "and in-run parity, side lines")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the in-run parity check")
    ap.add_argument("--no-side-lines", action="store_true",
                    help="with --full: skip the side lines and the CPU baseline (profiling runs: the kernel statistics then hold "
                         "the headline workload and the roofline's timings only)")
    ap.add_argument("--dry", action="store_true", help="launcher/harness rehearsal on CPU (gloo, no GPU work): prints the line with value 0")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (the fitted model and its predictions; "
                         "a fixed sample of K^-1) as DIR/<name>.npy, float64; rank 0 only")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.workload == "C3" and not args.dry:
        return run_c3(args)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        if os.environ.get("HBEGP_BENCH_CHILD"):
            print("bench.py: launched as a child without a torchrun environment", file=sys.stderr)
            sys.exit(2)
        sys.exit(self_launch(args))

    import numpy as np  # noqa: F401
    import torch  # noqa: F401  (loaded before libhbegp.so so the process holds one HIP runtime)

    from hbetune_rs_amd import dist as D

    rank, local_rank, world = D.rank_info()
    if args.gpus != world:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    dist = D.init("gloo" if args.dry else "nccl") if world > 1 else None

    if args.dry:
        # same barrier / max-over-ranks / rank-0 print as the real run, with a sleep for a step
        D.barrier(dist)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            time.sleep(0.01 * (1 + rank))
        D.barrier(dist)
        elapsed = D.max_over_ranks(dist, time.perf_counter() - t0)
        if rank == 0:
            print(json.dumps({"metric": "GP fit+predict/sec (n=4096,d=8,f64)", "value": 0.0, "unit": "fit+predict/s", "n_gpus": world,
                              "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
                              "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "none (dry run)",
                              "config": {"workload": "dry run of the launcher and timing harness"}}), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return

    from hbetune_rs_amd import gpr, synth

    w = synth.make_workload("M", n=args.n)
    X, y, theta = w["X"], w["y"], w["theta"]
    n, d = X.shape
    starts = synth.restart_points("M", w["lo"], w["hi"], N_RESTARTS)
    Xs = synth.candidates("M", M_CANDIDATES, d)

    ctx = gpr.Context(device_ids=[local_rank])
    fit_stats = {}

    def step(keep=False):
        fk = gpr.FittedKernel.new(X, y, w["theta0"], w["lo"], w["hi"], starts, nu=2.5, ctx=ctx, maxeval=EVALS_PER_RUN,
                                  fixed_work=True)
        fit_stats["n_evals"], fit_stats["n_not_pd"] = fk.n_evals, fk.n_not_pd
        mean, var, _ = fk.predict(Xs)
        fit_stats["model"] = {"theta": fk.theta.copy(), "lml": fk.lml, "mean": mean, "var": var}  # what the parity leg checks afterwards
        if keep:
            fit_stats["kept"] = fk  # --dump-outputs: the last timed model is read back and released after the timed region
        else:
            fk.release()
        return mean, var

    log(f"{args.warmup} warm-up + {args.steps} timed fit+predict steps")
    for _ in range(args.warmup):
        step()
    D.barrier(dist)
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(keep=bool(args.dump_outputs) and rank == 0 and i == args.steps - 1)
    D.barrier(dist)
    elapsed = D.max_over_ranks(dist, time.perf_counter() - t0)
    log(f"timed region done: {elapsed / args.steps * 1e3:.1f} ms per step")
    if "kept" in fit_stats:
        fk = fit_stats.pop("kept")
        tm = fit_stats["model"]
        dump_outputs(args.dump_outputs, dict(model_outputs(fk), mean=tm["mean"].astype(np.float64), var=tm["var"].astype(np.float64)))
        fk.release()

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = world * args.steps / elapsed  # whole-job fit+predict per second
        out = {
            "metric": "GP fit+predict/sec (n=4096,d=8,f64)",
            "value": value,
            "unit": "fit+predict/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": f"M: rosenbrock d={d} n={n} f64, Matern nu=5/2 x constant + white noise; fixed-work fit = "
                            f"{1 + N_RESTARTS} L-BFGS runs x {EVALS_PER_RUN} lml+gradient evaluations + K^-1, then predict "
                            f"mean+variance at m={M_CANDIDATES}",
                "evals_per_fit": fit_stats.get("n_evals"),
                "n_not_pd": fit_stats.get("n_not_pd"),
                "m_candidates": M_CANDIDATES,
                "parallelism": f"replicas x{world} (independent fits per GPU, no collective)",
            },
        }
        if args.full:
            log("roofline: kernel times with all slots evaluating at once")
            out["roofline"] = roofline_block(gpr, ctx, X, y, theta, 1 + N_RESTARTS, ms_per_step, fit_stats.get("n_evals", 0),
                                             2.0 * M_CANDIDATES * n * n, pmc_ok=args.n is None)
        if not args.full or args.no_side_lines:
            print(json.dumps(out), flush=True)
            if dist is not None:
                D.barrier(dist)
                dist.destroy_process_group()
            ctx.close()
            return
        # the same fit with the optimiser's own stopping rule (not timed above): evaluations it actually needs
        log("side lines: converged fit, f32, small n")
        t0 = time.perf_counter()
        fk = gpr.FittedKernel.new(X, y, w["theta0"], w["lo"], w["hi"], starts, nu=2.5, ctx=ctx, maxeval=EVALS_PER_RUN)
        t_conv = time.perf_counter() - t0
        out["converged_fit"] = {"seconds": t_conv, "evaluations": fk.n_evals, "n_not_pd": fk.n_not_pd, "lml": fk.lml,
                                "note": "early-stopping fit (projected-gradient / progress tolerances of csrc/lbfgsb.hpp), same data and starts"}
        fk.release()
        # --use-32 side line (C5: himmelblau d=2, n=2048, f32; main.rs:240-244): one evaluation, fp32 MFMA
        try:
            w5 = synth.make_workload("C5")
            th5 = w5["theta"].copy()
            p5 = gpr.Problem(w5["X"], w5["y"], nu=2.5, ctx=ctx)
            ph5 = p5.time_eval(th5, reps=5)
            p5.close()
            g64, m64 = ph5["gemm64_gflop"] + ph5["gemm128_gflop"], ph5["gemm64_ms"] + ph5["gemm128_ms"]
            out["f32_side_line"] = {"workload": "C5: himmelblau d=2 n=2048 f32, one lml+gradient evaluation, single stream",
                                    "eval_ms": ph5["eval_graph_ms"],
                                    "eval_frac_of_fp32_peak": 2048 ** 3 * 1e-12 / (ph5["eval_graph_ms"] * 1e-3) / PEAK_FP32_MFMA_TFLOPS,
                                    "dag_kernel<float> TFLOP/s (task queue: factor + inverse + K^-1)": (ph5["dag_gflop"] / ph5["dag_ms"]) if ph5["dag_ms"] > 0 else None,
                                    "gemm_kernel<float> 64/128-tile TFLOP/s": (g64 / m64) if m64 > 0 else None,
                                    "gemm_kernel<float> 32-tile TFLOP/s": (ph5["gemm32_gflop"] / ph5["gemm32_ms"]) if ph5["gemm32_ms"] > 0 else None,
                                    "peak_fp32_mfma": PEAK_FP32_MFMA_TFLOPS}
            # does --use-32 buy a user anything?  fixed-work fits (3 runs x 150 evaluations), f32 beside f64 on the same data
            def fit_rate(ww, dtype, reps=2):
                Xd, yd = ww["X"].astype(dtype), ww["y"].astype(dtype)
                st = synth.restart_points(ww["name"], ww["lo"], ww["hi"], N_RESTARTS)
                best = None
                log(f"  fit rate {ww['name']} n={ww['n']} {np.dtype(dtype).name}")
                for _ in range(reps + 1):  # first one warms the plan cache / pools
                    t0 = time.perf_counter()
                    f = gpr.FittedKernel.new(Xd, yd, ww["theta0"], ww["lo"], ww["hi"], st, nu=2.5, ctx=ctx, maxeval=EVALS_PER_RUN, fixed_work=True)
                    dt = time.perf_counter() - t0
                    f.release()
                    best = dt if best is None else min(best, dt)
                return 1.0 / best

            import numpy as np

            out["f32_side_line"]["fits_per_s"] = {
                "C5 n=2048 d=2 f32": fit_rate(w5, np.float32), "C5 n=2048 d=2 f64": fit_rate(w5, np.float64),
                "M n=4096 d=8 f32": fit_rate(w, np.float32, reps=1), "M n=4096 d=8 f64": value / world,
                "note": "fixed-work fits, 3 optimiser runs x 150 evaluations, best of the timed repetitions; M f64 is the headline (incl. predict)"}
        except Exception as e:  # the side line must never cost the headline
            out["f32_side_line"] = {"error": str(e)}
        # the other BASELINE configurations at their full size (C3 is --workload C3, C5 the f32 line above): one evaluation alone
        # and a fixed-work fit each, f64
        try:
            cfgs = {}
            for cname in ("C1", "C2", "C4"):
                log(f"  BASELINE config {cname}")
                wc = synth.make_workload(cname)
                pc = gpr.Problem(wc["X"], wc["y"], nu=2.5, ctx=ctx)
                phc = pc.time_eval(wc["theta"], reps=5)
                pc.close()
                stc = synth.restart_points(cname, wc["lo"], wc["hi"], N_RESTARTS)
                best = None
                for _ in range(2):
                    t0 = time.perf_counter()
                    f = gpr.FittedKernel.new(wc["X"], wc["y"], wc["theta0"], wc["lo"], wc["hi"], stc, nu=2.5, ctx=ctx, maxeval=EVALS_PER_RUN, fixed_work=True)
                    dt = time.perf_counter() - t0
                    f.release()
                    best = dt if best is None else min(best, dt)
                nn = wc["X"].shape[0]
                cfgs[f"{cname} n={nn} d={wc['X'].shape[1]}"] = {
                    "eval_ms": phc["eval_graph_ms"], "fits_per_s": 1.0 / best,
                    "fit_frac_of_fp64_peak": (N_RESTARTS + 1) * EVALS_PER_RUN * nn ** 3 * 1e-12 / best / PEAK_FP64_MFMA_TFLOPS}
            out["baseline_configs_side_line"] = dict(cfgs, note="BASELINE.json configs[0], [1], [3] at full size, f64: one lml+gradient evaluation alone "
                                                                "(graph replay) and fixed-work fits (3 runs x 150 evaluations, best of 2); parity at these sizes: "
                                                                "tests/test_gpu_fullsize.py, tests/test_gpu_parity.py")
        except Exception as e:
            out["baseline_configs_side_line"] = {"error": str(e)}
        # small and mid n (the reference's own regime is n <= 200, minimize.rs:118-120): fixed-work fits/s, f64
        try:
            small = {}
            for ns in (100, 128, 256, 512, 1024):
                log(f"  small n: {ns}")
                wn = synth.make_workload("M", n=ns)
                stn = synth.restart_points("M", wn["lo"], wn["hi"], N_RESTARTS)
                best = None
                for _ in range(3):
                    t0 = time.perf_counter()
                    f = gpr.FittedKernel.new(wn["X"], wn["y"], wn["theta0"], wn["lo"], wn["hi"], stn, nu=2.5, ctx=ctx, maxeval=EVALS_PER_RUN, fixed_work=True)
                    dt = time.perf_counter() - t0
                    f.release()
                    best = dt if best is None else min(best, dt)
                small[f"n={ns}"] = {"fits_per_s": 1.0 / best, "evals_per_s": (1 + N_RESTARTS) * EVALS_PER_RUN / best,
                                    "frac_of_fp64_peak": (1 + N_RESTARTS) * EVALS_PER_RUN * ns ** 3 * 1e-12 / best / PEAK_FP64_MFMA_TFLOPS}
            out["small_n_side_line"] = dict(small, note="config M data cut to n rows, d=8, f64, 3 runs x 150 evaluations, best of 3 fits; up to n=128 "
                                            "(the reference's own regime, minimize.rs:118-120) every optimiser run is one persistent launch "
                                            "(evaluation + L-BFGS step on the device)")
        except Exception as e:
            out["small_n_side_line"] = {"error": str(e)}
        if world == 1 and not args.no_side_lines:
            # replicas on ONE GPU: k independent fits side by side, one host thread each, in a child
            # process of its own, with the runtime's hardware-queue settings as this process has them
            try:
                conc = {}
                for nn_, ks_ in ((128, "1 4 16"), (1024, "1 4")):
                    cp = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "concurrent_fits.py"), str(nn_)] + ks_.split(),
                                        capture_output=True, text=True, timeout=300)
                    last = [l for l in cp.stdout.splitlines() if l.startswith("{")]
                    conc[f"n={nn_}"] = json.loads(last[-1]) if last else {"error": (cp.stderr or cp.stdout)[-300:]}
                out["concurrent_fits_side_line"] = dict(conc, note="aggregate fixed-work fits/s of k host threads fitting on one context / one GPU (config M "
                                                        "data cut to n rows, 3 runs x 150 evaluations each), hardware queues as the bench process has them; every concurrent fit is "
                                                        "compared bit for bit with the same fit alone")
            except Exception as e:
                out["concurrent_fits_side_line"] = {"error": str(e)}
        parity_failed = False
        if world == 1 and not args.no_cpu_baseline:
            par = {}

            def parity(O, ref):
                log("parity: the GPU's evaluation, model and the timed model next to the oracle")
                par.update(parity_in_run(gpr, ctx, w, theta, Xs, fit_stats.get("model"), O, ref))

            cb = cpu_baseline(w, theta, Xs, fit_stats.get("n_evals") or (1 + N_RESTARTS) * EVALS_PER_RUN, parity=parity)
            out["cpu_baseline"] = cb
            out["speedup_vs_cpu_port"] = value / cb["value"]
            out["parity_in_run"] = par
            parity_failed = not par.get("ok", False)
        print(json.dumps(out), flush=True)
        if parity_failed:
            log(f"PARITY FAILED: {json.dumps(out['parity_in_run'])}")
            if dist is not None:
                dist.destroy_process_group()
            ctx.close()
            sys.exit(3)
    if dist is not None:
        D.barrier(dist)
        dist.destroy_process_group()
    ctx.close()


if __name__ == "__main__":
    main()
