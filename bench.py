#!/usr/bin/env python3
"""Benchmark of the VideoPose3D temporal-model hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]

Workload (BASELINE.json `metric`: "frames/sec (fwd+bwd) 243-frame arc=3,3,3,3,3 B=1024"):
  one step = one training pass (forward + backward incl. BatchNorm statistics and dropout p=0.25) of
  TemporalModelOptimized1f, arc 3,3,3,3,3, C=1024, over one synthetic batch of B=1024 RF-length (243-frame)
  windows that is already resident in HBM; for N>1 one such batch PER RANK (weak scaling, global batch
  N*1024) plus the flat-gradient sum all-reduce over RCCL.  frames/s = predicted frames (= batch elements) per
  second, whole job.  The optimizer is torch.optim.Adam in run.py (out of scope) and is NOT in the timed
  region; its cost is reported separately (`adam_ms`).
Arithmetic: the headline runs the library default, "f16x3" = split-fp16 operands on v_mfma_f32_32x32x16_f16 with fp32
accumulation (fp32-class results: 22+ operand bits, exact products; same parity tests and tolerances as the fp32 path);
the same step on the exact-fp32 MFMA kernels (math "f32", v_mfma_f32_32x32x2_f32) is timed next to it (`f32_mfma`).
Rank 0 prints ONE JSON line on stdout, <= 2 KB (final_line): the contract's fields + roofline + cpu_baseline + mpjpe_vs_ref +
f32_mfma + cfg2_eval_fwd.  Everything else measured here (per-launch tables, streaming kernels, per-step timings, drop-in /
hipGraph / PyTorch-ROCm sections) is written to bench_detail.json next to this file (and to gpurun_out/ when that exists).
Sections of the record:
  cfg2_eval_fwd : BASELINE.json configs[1] -- TemporalModel eval forward, B=1024, T=243 (5.34 TFLOP / call)
  roofline      : dominant GEMM kernel family of the step, algorithmic FLOPs / HIP-event launch durations
  cpu_baseline  : the reference's CPU path (ATen/oneDNN through oracle/torch_cpu_path.py, kind "port") on this
                  host's cores, bounded sample of the same workload; mpjpe_vs_ref = HIP vs that path on the sample
  rocm_reference_baseline : the same reference path executed by PyTorch-ROCm (MIOpen) on this GPU, B=1024 (N=1 only)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# Before the HIP runtime initialises: kernel arguments in device memory -- the step is a dependent chain of ~200 launches,
# -2.6 ... -3.9 % step time (profiles/r05_dev_kernarg_ab.txt).  Set HERE, in the launcher, not by importing the package (round 6:
# a library must not change its host process's environment); it also covers every baseline leg of this process, and the ranks
# that relaunch_under_torchrun starts inherit it.  A value already in the environment wins; the line reports what was in effect.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

FW = [3, 3, 3, 3, 3]
C = 1024
B = 1024
RF = 243
PEAK_F32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CUs x 4 SIMD x 64 FLOP/clk x 2.4 GHz
PEAK_F16_MFMA_TFLOPS = 2500.0         # MI355X_MICROARCH.md: dense f16/bf16 MFMA (v_mfma_f32_32x32x16_f16: 1024 FLOP/clk/SIMD)
MFMA_PER_MAC_F16X3 = 3                # the split scheme issues ah*bh + ah*bl + al*bh: 3 executed MFMA FLOPs per algorithmic FLOP
SUSTAINED_F16_MFMA_TFLOPS = 1700.0    # what a bare v_mfma_f32_32x32x16_f16 loop sustains on RANDOM operands on this chip (DVFS /
                                      # power: tools/ubench/mfma_peak.hip measured 1,697-1,703 TFLOP/s with 1 and 2 workgroups per
                                      # CU, with and without a barrier every 24 MFMAs) -- the practical ceiling of the matrix pipes
ACHIEVABLE_HBM_GBPS = 6300.0           # MI355X_MICROARCH.md: what a streaming kernel sustains of the 8 TB/s HBM3E peak
FLOP_TRAIN_PER_FRAME = 1023866880     # fwd 352,569,344 + bwd 671,297,536 (conv MACs x 2)
FLOP_EVAL_PER_FRAME = 5217830912      # TemporalModel forward on a 243-frame window


DETAIL_FILE = "bench_detail.json"
FINAL_LINE_MAX = 2048


def _r(v, nd=4):
    """Round floats for the final line (the side file keeps full precision)."""
    if isinstance(v, float):
        return float("%.*g" % (nd + 2, v))
    return v


def final_line(out):
    """The ONE stdout line the driver parses: <= FINAL_LINE_MAX bytes, exactly the fields of the bench contract (metric .. config,
    roofline, cpu_baseline) plus the three precision-matched companions.  Everything else `main` measured -- per-launch tables,
    streaming kernels, per-step timings, the drop-in / hipGraph / PyTorch-ROCm sections and all prose -- goes to DETAIL_FILE
    (BENCH_r04: a 20 KB line was not parsed by the driver)."""
    def pick(d, keys):
        return {k: _r(d[k]) for k in keys if d is not None and k in d}
    line = {k: _r(out.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                        "scaling", "vs_baseline", "dtype", "math", "data")}
    line["config"] = out.get("config")
    roof = out.get("roofline")
    if roof:
        line["roofline"] = pick(roof, ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes", "kernel",
                                       "launches_per_step", "avg_launch_ms"))
        if isinstance(line["roofline"].get("kernel"), str):
            line["roofline"]["kernel"] = line["roofline"]["kernel"].split(" (")[0]
    cb = out.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = pick(cb, ("value", "unit", "cores", "kind"))
        line["cpu_baseline"]["sample"] = str(cb.get("sample", ""))[:160]
    if out.get("mpjpe_vs_ref"):
        line["mpjpe_vs_ref"] = pick(out["mpjpe_vs_ref"], ("value", "tolerance", "sample_b"))
    line["step_frac_of_roofline"] = _r(out.get("step_frac_of_roofline"))
    if out.get("launches_per_step"):
        line["launches_per_step"] = out["launches_per_step"]["libvp3d"]
    if out.get("f32_mfma"):
        line["f32_mfma"] = pick(out["f32_mfma"], ("value", "ms_per_step", "step_frac_of_fp32_mfma_peak"))
    ev = out.get("cfg2_eval_fwd")
    if ev:
        line["cfg2_eval_fwd"] = {"ms": _r(ev["ms"]), "tflops": _r(ev["tflops"]), "frac": _r(ev.get("frac")), "math": ev.get("math")}
    ev32 = out.get("cfg2_eval_fwd_f32_mfma")
    if ev32:
        line["cfg2_eval_fwd_f32_mfma"] = {"ms": _r(ev32["ms"]), "frac": _r(ev32.get("frac"))}
    ref = out.get("rocm_reference_baseline")
    if ref and "value" in ref:
        line["rocm_reference"] = {"value": _r(ref["value"]), "speedup": _r(out.get("speedup_vs_rocm_reference"))}
    c5 = out.get("cfg5_semi_supervised_step")
    if c5:
        line["cfg5_ms"] = pick(c5, ("ms_per_step", "graph_replay_ms_per_step"))
    if out.get("range_guard") is not None:
        line["range_guard"] = out["range_guard"]
    if out.get("box") and "error" not in out["box"]:
        line["box"] = pick(out["box"], ("power_w", "power_cap_w", "sclk_mhz", "temp_junction_c"))
    for k in ("value_path", "dry_run", "barrier_to_barrier_s"):
        if k in out:
            line[k] = _r(out[k])
    la = out.get("launcher")
    if la:
        line["launcher"] = {"rccl_env": la.get("rccl_env")}
        if out.get("dry_run"):
            line["launcher"]["cores_per_rank"] = la.get("cores_per_rank")
        elif la.get("cores_of_rank0") is not None:
            line["launcher"]["n_cores_of_rank0"] = len(la["cores_of_rank0"])
    if "eager" in out:
        line["eager"] = pick(out["eager"], ("value", "ms_per_step"))
    line["env"] = {"HIP_FORCE_DEV_KERNARG": os.environ.get("HIP_FORCE_DEV_KERNARG")}
    line["detail"] = out.get("detail_file")
    s = json.dumps(line, separators=(",", ":"))
    for k in ("box", "launcher", "cfg5_ms", "rocm_reference", "cfg2_eval_fwd_f32_mfma", "range_guard", "step_frac_of_roofline"):   # never reached today:
        if len(s) <= FINAL_LINE_MAX:                                                                           # the contract's
            break                                                                                              # fields stay
        line.pop(k, None)
        s = json.dumps(line, separators=(",", ":"))
    assert len(s) <= FINAL_LINE_MAX, len(s)
    return s


def write_detail(out):
    """Full measurement record next to bench.py (and under gpurun_out/ when that exists, so that it travels back)."""
    paths = [os.path.join(ROOT, DETAIL_FILE)]
    if os.path.isdir(os.path.join(ROOT, "gpurun_out")):
        paths.append(os.path.join(ROOT, "gpurun_out", DETAIL_FILE))
    written = None
    for p in paths:
        try:
            with open(p, "w") as f:
                json.dump(out, f, indent=1)
            written = written or os.path.relpath(p, ROOT)
        except OSError:
            continue
    return written


def synthetic_batch(batch, gen):
    x = (torch.randn(batch, RF, 17, 2, generator=gen) * 0.5).clamp(-1, 1)      # screen-normalised keypoints
    tgt = torch.randn(batch, 1, 17, 3, generator=gen) * 0.3
    tgt[:, :, 0] = 0                                                            # run.py:407
    return x, tgt


def mpjpe(pred, target):                                                        # loss.py:11-17
    return torch.mean(torch.norm(pred - target, dim=len(target.shape) - 1))


def _latest(*names):
    """The newest committed collection of a profile that exists (tools/profile_round.sh <tag> writes <tag>_*)."""
    for n in names:
        p = os.path.join(ROOT, "profiles", n)
        if os.path.exists(p):
            return p
    return os.path.join(ROOT, "profiles", names[-1])


PMC_JSON = {"f32": _latest("r06f32_pmc_traffic.json", "r05f32_pmc_traffic.json", "r04f32_pmc_traffic.json"),
            "f16x3": _latest("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json")}
FAMILY_KERNELS = {"f32": {"tconv_fwd": "k_rows_gemm<true,", "tconv_dgrad": "k_rows_gemm<false,", "tconv_wgrad": "k_red_gemm<"},
                  # one kernel serves all three GEMM forms of the split-fp16 path (all are "NT")
                  "f16x3": {"tconv_fwd": "k_nt_s16<", "tconv_dgrad": "k_nt_s16<", "tconv_wgrad": "k_nt_s16<"}}


STEP_TABLE_JSON = {"f16x3": _latest("r06_step_table.json", "r05_step_table.json", "r04_step_table.json"),
                   "f32": _latest("r06f32_step_table.json", "r05f32_step_table.json", "r04f32_step_table.json")}


def pmc_traffic(family, math):
    """Per-launch table first (profiles/r05_step_table.json: every GEMM launch of the step with its own FETCH_SIZE x2 +
    WRITE_SIZE): the family's traffic is the mean over ITS launches, comparable with `algorithmic_bytes`; else the
    per-kernel-template means of the older profile."""
    path = STEP_TABLE_JSON.get(math)
    if path:
        try:
            with open(path) as f:
                rows = [r for r in json.load(f)["launches"] if r["family"] == family and r["fetch_bytes"] is not None]
            if rows:
                return (sum(r["fetch_bytes"] + r["write_bytes"] for r in rows) / len(rows),
                        "bytes per launch (L2<->fabric: FETCH_SIZE x2 + WRITE_SIZE, Infinity-Cache hits included), mean over the "
                        "%d %s launches of one step in %s (algorithmic mean of the same launches: %.1f MB)"
                        % (len(rows), family, os.path.relpath(path, ROOT), sum(r["algorithmic_bytes"] for r in rows) / len(rows) / 1e6))
        except (OSError, ValueError, KeyError):
            pass
    return _pmc_traffic_templates(family, math)


def pmc_traffic_of_cfg(cfg, math, live=None):
    """The same per-launch table, the launches served by one kernel (tile configuration `cfg`).  live: this run's launches of
    that kernel as (M, N, K, k_slices) -- the committed table is only quoted when it holds EXACTLY those launches (a planner or
    kernel change since the profile was collected would otherwise put another kernel's bytes beside this run's time)."""
    path = STEP_TABLE_JSON.get(math)
    try:
        with open(path) as f:
            rows = [r for r in json.load(f)["launches"] if r["cfg"] == cfg and r["fetch_bytes"] is not None]
    except (OSError, ValueError, KeyError, TypeError):
        return None, None
    if not rows:
        return None, ("the committed per-launch table %s has no launches of tile configuration %s: collected before this "
                      "kernel served them (tools/profile_round.sh re-collects)" % (os.path.relpath(path, ROOT), cfg))
    if live is not None:
        have = sorted((r["M"], r["N"], r["K"], r["k_slices"]) for r in rows)
        if have != sorted(live):
            return None, ("the committed per-launch table %s is stale for tile configuration %s: it holds launches %s, this run "
                          "issued %s (tools/profile_round.sh re-collects)" % (os.path.relpath(path, ROOT), cfg, have, sorted(live)))
    return (sum(r["fetch_bytes"] + r["write_bytes"] for r in rows) / len(rows),
            "bytes per launch (L2<->fabric: FETCH_SIZE x2 + WRITE_SIZE, Infinity-Cache hits included), mean over the %d launches of "
            "this kernel in one step, %s (algorithmic mean of the same launches: %.1f MB; the table's launch list was checked "
            "against this run's)"
            % (len(rows), os.path.relpath(path, ROOT), sum(r["algorithmic_bytes"] for r in rows) / len(rows) / 1e6))


def _pmc_traffic_templates(family, math):
    """HBM-side bytes per launch of a GEMM family from the committed rocprofv3 PMC passes of THIS command
    (profiles/r04*_pmc_traffic.json: FETCH_SIZE and WRITE_SIZE collected in separate runs, FETCH_SIZE doubled per the
    gfx950 correction of MI355X_MICROARCH.md; tools/pmc_traffic.py).  PMC counters cannot be read from inside the
    timed process, so the value is the committed measurement, averaged over the family's launches like `achieved`."""
    path = PMC_JSON[math]
    try:
        with open(path) as f:
            tab = json.load(f)["kernels"]
    except (OSError, ValueError, KeyError):
        return None, "no committed PMC profile found (%s)" % os.path.relpath(path, ROOT)
    key = FAMILY_KERNELS[math][family].replace(" ", "")
    tot = n = 0.0
    for name, t in tab.items():
        if key in name.replace(" ", ""):
            launches = max(t["launches_fetch_pass"], t["launches_write_pass"], 1)
            tot += t["hbm_bytes_per_launch"] * launches
            n += launches
    if not n:
        return None, "kernel family not present in %s" % os.path.relpath(path, ROOT)
    return tot / n, ("bytes per launch (L2<->fabric: FETCH_SIZE x2 + WRITE_SIZE, Infinity-Cache hits included), mean "
                     "over the %d launches of %s in %s" % (int(n), key, os.path.relpath(path, ROOT)))


def usable_cores():
    """Logical CPUs this process may actually run on: min(cpu_count, affinity mask, cgroup cpu quota)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(int(parts[0]) / int(parts[1]))))
            else:
                q = int(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                        n = min(n, max(1, int(q / int(f.read()))))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def cpu_baseline(dev, budget_s=4.0):
    """The reference's CPU path timed on this host's cores, next to the GPU number.

    /root/reference does not exist on the GPU box, so the timed code is oracle/torch_cpu_path.py: the same
    ATen/oneDNN kernels the reference's nn.Conv1d/BatchNorm1d/ReLU modules + autograd run on a CPU, wired as
    model.py:187-197 (kind "port"; pinned to reference-generated goldens by tests/test_oracle_golden.py).
    Bounded sample: the batch is sized so that one fwd+bwd takes ~budget_s seconds (CPU throughput is B-linear).
    The same leg is the checker for the metric's "MPJPE vs ref": HIP output vs this CPU path on the sample."""
    from oracle import torch_cpu_path as T
    from videopose3d_amd import TemporalModelOptimized1f
    cores = usable_cores()
    torch.manual_seed(0)
    m = TemporalModelOptimized1f(17, 2, 17, FW, dropout=0.0, channels=C).to(dev).train()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    gen = torch.Generator().manual_seed(1234)

    def run(bsz, iters, dropout=0.25):
        """dropout 0.25 = the workload of the GPU headline (timed); 0.0 for the MPJPE comparison (torch's mask stream is not ours)"""
        x, tgt = synthetic_batch(bsz, gen)
        ts, out = [], None
        for _ in range(iters):
            sdi = {k: v.clone() for k, v in sd.items()}
            t0 = time.perf_counter()
            _, out, _ = T.train_step(sdi, x, tgt, FW, kind="strided", dropout=dropout)
            ts.append(time.perf_counter() - t0)
        return x, out, ts

    # Thread count: the box reports more logical CPUs than the container may use; oversubscribed oneDNN threads
    # spin on each other (measured: 256 threads -> 25 s for a batch 8 threads finish in 0.13 s).  Walk the thread
    # count up from 8 and keep the fastest (stop at the first regression) -- `cores` reports what was used.
    best_t, best_dt, n = None, None, 8
    while n <= cores or best_t is None:
        n = min(n, cores)
        torch.set_num_threads(n)
        _, _, ts = run(32, 2)
        if best_dt is not None and ts[-1] > best_dt:
            break
        best_t, best_dt = n, ts[-1]
        if n == cores:
            break
        n *= 2
    torch.set_num_threads(best_t)
    _, _, ts = run(32, 2)                                   # warm-up + calibration at the chosen thread count
    bsz = int(min(B, max(32, round(32 * budget_s / ts[-1] / 32) * 32)))
    _, _, ts = run(bsz, 4)
    dt = float(np.mean(ts[1:]))
    x, y_cpu, _ = run(bsz, 1, dropout=0.0)               # (un-timed) the deterministic forward both paths can be compared on
    with torch.no_grad():
        y_gpu = m(x.to(dev)).cpu()
    err = float(mpjpe(y_gpu, y_cpu))
    try:
        with open("/proc/cpuinfo") as f:
            cpu_name = next((l.split(":", 1)[1].strip() for l in f if l.startswith("model name")), "?")
    except OSError:
        cpu_name = "?"
    base = dict(value=bsz / dt, unit="frames/s", cores=int(torch.get_num_threads()), kind="port",
                sample="cfg3 train step fwd+bwd (dropout 0.25) on oracle/torch_cpu_path.py (ATen/oneDNN), B=%d, 3 iters x %.1f s, %d threads, %s"
                       % (bsz, dt, best_t, cpu_name),
                sample_detail="oracle/torch_cpu_path.py (ATen/oneDNN conv1d/batch_norm/relu + autograd = what the reference "
                       "runs on CPU), TemporalModelOptimized1f arc 3,3,3,3,3 C=1024 train fwd+bwd, BN statistics, dropout 0.25 (the headline's workload), "
                       "B=%d x 243 frames, 3 timed iters after 1 warm-up, %.2f s/iter, %d threads (fastest of a 8,16,.. sweep); "
                       "host: %d logical CPUs (%d usable by this container), %s"
                       % (bsz, dt, best_t, os.cpu_count() or 0, cores, cpu_name))
    return base, dict(value=err, unit="mpjpe (output units = metres) between the HIP path and the CPU reference path",
                      sample_b=bsz, tolerance=1e-3)


def rocm_reference_baseline(dev, x, tgt):
    """Second baseline ("optional second comparator"): the reference's own execution path -- the
    torch.nn.functional conv1d / batch_norm / relu / dropout + autograd wiring of oracle/torch_cpu_path.py, i.e. what
    run.py executes with the reference classes -- run by PyTorch-ROCm (MIOpen / rocBLAS) on THIS GPU, same shapes, same
    batch.  This is "the reference on MI355X"; like cpu_baseline it is a baseline leg, never the product path."""
    from oracle import torch_cpu_path as T
    from videopose3d_amd import TemporalModelOptimized1f
    torch.manual_seed(0)
    m = TemporalModelOptimized1f(17, 2, 17, FW, dropout=0.25, channels=C)
    sd = {k: v.detach().to(dev) for k, v in m.state_dict().items()}
    t0 = time.perf_counter()
    for _ in range(2):                                                   # MIOpen's kernel search happens here
        T.train_step(sd, x, tgt, FW, kind="strided", dropout=0.25)
    torch.cuda.synchronize()
    t_find = time.perf_counter() - t0
    t0 = time.perf_counter()
    n = 5
    for _ in range(n):
        T.train_step(sd, x, tgt, FW, kind="strided", dropout=0.25)
    torch.cuda.synchronize()
    ms_train = (time.perf_counter() - t0) / n * 1e3
    with torch.no_grad():
        for _ in range(2):
            T.forward(sd, x, FW, kind="dilated", training=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            T.forward(sd, x, FW, kind="dilated", training=False)
        torch.cuda.synchronize()
        ms_eval = (time.perf_counter() - t0) / 3 * 1e3
    return {"what": "the reference's module stack (F.conv1d / F.batch_norm / relu / dropout + autograd, oracle/torch_cpu_path.py) "
                    "executed by PyTorch-ROCm (MIOpen / rocBLAS, fp32) on this GPU: cfg3 train step and cfg2 eval forward, B=1024",
            "value": B / ms_train * 1e3, "unit": "frames/s", "train_ms_per_step": ms_train, "cfg2_eval_ms": ms_eval,
            "cfg2_eval_frames_per_s": B / ms_eval * 1e3, "torch": torch.__version__,
            "first_two_steps_s": t_find}


def box_state(step, dev_index=0, n_steps=80, samples=12, sysfs="/sys"):
    """Power / clock / temperature of THIS box's GPU while the step runs (sysfs hwmon of the amdgpu device; read-only, < 1 ms per
    sample): `n_steps` steps are enqueued, the files are sampled while the GPU works through them.  Freshly leased MI355X boxes of
    round 5 differed by 12 % on every split-fp16 number and 1.4 % on the exact-fp32 engine (profiles/r05_bench_lines.txt): the
    sustained MFMA clock under the board's power limit is a property of the box, and this puts it on record next to `value`."""
    import glob
    cands = sorted(glob.glob(os.path.join(sysfs, "class/drm/card*/device/hwmon/hwmon*")))
    if not cands:
        return {"error": "no amdgpu hwmon in sysfs"}
    # sysfs lists every GPU of the node, the process sees one: match by PCI address (card*/device -> .../<domain>:<bus>:<dev>.0)
    hw, how = None, "pci address"
    try:
        pr = torch.cuda.get_device_properties(dev_index)
        want = "%04x:%02x:%02x." % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        for c in cands:
            if want in os.path.realpath(os.path.join(c, "..", "..")):
                hw = c
    except Exception:  # noqa: BLE001
        pass

    def rd(name):
        try:
            with open(os.path.join(hw, name)) as f:
                return float(f.read().strip())
        except (OSError, ValueError):
            return None
    for _ in range(n_steps):
        step()
    if hw is None:                                   # no PCI match: the card that draws the most power right now
        how = "highest power draw"
        time.sleep(0.05)
        best = -1.0
        for c in cands:
            for name in ("power1_average", "power1_input"):
                try:
                    with open(os.path.join(c, name)) as f:
                        v = float(f.read().strip())
                    if v > best:
                        best, hw = v, c
                    break
                except (OSError, ValueError):
                    continue
        if hw is None:
            hw = cands[0]
    acc = {"power_w": [], "sclk_mhz": [], "temp_junction_c": []}
    for _ in range(samples):
        time.sleep(0.02)
        p = rd("power1_average")
        if p is None:
            p = rd("power1_input")
        f, t = rd("freq1_input"), rd("temp2_input")
        if p is not None:
            acc["power_w"].append(p / 1e6)
        if f is not None:
            acc["sclk_mhz"].append(f / 1e6)
        if t is not None:
            acc["temp_junction_c"].append(t / 1e3)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    out = {k: (round(sum(v) / len(v), 1) if v else None) for k, v in acc.items()}
    cap = rd("power1_cap")
    out["power_cap_w"] = round(cap / 1e6, 1) if cap is not None else None
    out["hwmon"], out["matched_by"] = hw, how
    out["what"] = "mean of %d sysfs samples taken while %d steps of the headline workload were executing" % (samples, n_steps)
    return out


def semi_supervised_step_latency(dev):
    """BASELINE.json configs[4]: run.py's semi-supervised step (run.py:322-394) -- pose + trajectory models (arc 3,3,3,
    C=1024), 64 labelled + 64 unlabelled 27-frame windows, mpjpe + weighted trajectory loss + back-projection through
    project_to_2d (HIP) + bone-length term -- forward + backward of both models, step latency.  Launch-latency-bound at this
    size, so the models stay on the fp32 kernels (engine.use_s16's size threshold)."""
    from videopose3d_amd import TemporalModelOptimized1f
    from videopose3d_amd import loss as vloss
    from videopose3d_amd.camera import project_to_2d
    fw, bsz = [3, 3, 3], 64
    torch.manual_seed(0)
    pos = TemporalModelOptimized1f(17, 2, 17, fw, dropout=0.25, channels=C).to(dev).train()
    traj = TemporalModelOptimized1f(17, 2, 1, fw, dropout=0.25, channels=C).to(dev).train()
    gen = torch.Generator().manual_seed(5)
    x_l = (torch.randn(bsz, 27, 17, 2, generator=gen) * 0.5).clamp(-1, 1).to(dev)
    x_u = (torch.randn(bsz, 27, 17, 2, generator=gen) * 0.5).clamp(-1, 1).to(dev)
    y3 = (torch.randn(bsz, 1, 17, 3, generator=gen) * 0.3).to(dev)
    y3[:, :, 0, 2] = y3[:, :, 0, 2].abs() + 3.0                                  # a trajectory in front of the camera
    cam = torch.tensor([1.15, 1.15, 0.0, 0.0, -0.2, 0.25, 0.0, 0.0, 0.0]).repeat(bsz, 1).to(dev)
    parents = torch.tensor([0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15], device=dev)      # parents of joints 1..16
    y_traj = y3[:, :, :1].clone()
    y_pos = y3.clone()
    y_pos[:, :, 0] = 0
    cat = torch.cat((x_l, x_u), dim=0)
    target = x_u[:, 13:-13, :, :2].contiguous()

    def step():
        pos.zero_grad(set_to_none=True)
        traj.zero_grad(set_to_none=True)
        step_fn()

    def step_fn():
        p_cat, t_cat = pos(cat), traj(cat)
        loss = vloss.mpjpe(p_cat[:bsz], y_pos) + vloss.weighted_mpjpe(t_cat[:bsz], y_traj, 1 / y_traj[:, :, :, 2])
        recon = project_to_2d(p_cat[bsz:] + t_cat[bsz:], cam)
        loss = loss + vloss.mpjpe(recon, target)
        dists = p_cat[:, :, 1:] - p_cat.index_select(2, parents)
        bone = torch.mean(torch.norm(dists, dim=3), dim=1)
        loss = loss + torch.mean(torch.abs(torch.mean(bone[:bsz], dim=0) - torch.mean(bone[bsz:], dim=0)))
        loss.backward()
        return loss.detach()

    def timed(fn, n=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    ms = timed(step)
    out = {"workload": "cfg5: semi-supervised step, arc 3,3,3 C=1024, pose + trajectory models, 64 labelled + 64 unlabelled "
                       "windows, mpjpe + weighted mpjpe + project_to_2d back-projection + bone-length loss, fwd + bwd",
           "ms_per_step": ms, "math": "f32 kernels (below the split-fp16 engine's size threshold)"}
    try:
        # the same step as ONE hipGraph replay (graph.GraphedStep: autograd + torch ops + HIP kernels captured once)
        from videopose3d_amd.graph import GraphedStep
        g = GraphedStep(step_fn, models=(pos, traj))
        out["graph_replay_ms_per_step"] = timed(lambda: g())
        out["graph_speedup"] = ms / out["graph_replay_ms_per_step"]
    except Exception as e:                                # the eager number stands on its own
        out["graph_replay_error"] = repr(e)[:200]
    return out


def instrumented(step, ops, n_prof, math):
    """Per-kernel-family roofline, measured live with HIP events on the launch stream around every C-ABI GEMM call."""
    recs = []
    ops.set_profiler(recs)
    for _ in range(n_prof):
        step()
    torch.cuda.synchronize()
    ops.set_profiler(None)
    fam, shapes, streams = {}, {}, {}
    for name, flops, e0, e1, nbytes, shape in recs:
        ms = e0.elapsed_time(e1)
        if name.startswith("stream_"):                 # HBM-bound producers: bytes / time, not part of the GEMM families
            f = streams.setdefault((name, shape), dict(bytes=0.0, ms=0.0, calls=0))
            f["bytes"] += nbytes
            f["ms"] += ms
            f["calls"] += 1
            continue
        f = fam.setdefault(name, dict(flops=0.0, ms=0.0, calls=0, bytes=0.0))
        f["flops"] += flops
        f["bytes"] += nbytes
        f["ms"] += ms
        f["calls"] += 1
        g = shapes.setdefault((name, shape), dict(flops=0.0, ms=0.0, calls=0, bytes=0.0))
        g["flops"] += flops
        g["bytes"] += nbytes
        g["ms"] += ms
        g["calls"] += 1
    kernels = {k: dict(calls_per_step=v["calls"] // n_prof, ms_per_step=v["ms"] / n_prof,
                       avg_launch_ms=v["ms"] / v["calls"], tflops=v["flops"] / v["ms"] / 1e9,
                       algorithmic_bytes_per_launch=v["bytes"] / v["calls"])
               for k, v in fam.items()}
    peak_alg = PEAK_F16_MFMA_TFLOPS / MFMA_PER_MAC_F16X3 if math == "f16x3" else PEAK_F32_MFMA_TFLOPS
    per_launch = []
    for (name, shape), v in shapes.items():
        row = {"family": name, "calls_per_step": v["calls"] / n_prof, "us": v["ms"] / v["calls"] * 1e3,
               "tflops": v["flops"] / v["ms"] / 1e9, "frac_of_peak": v["flops"] / v["ms"] / 1e9 / peak_alg,
               "algorithmic_MB": v["bytes"] / v["calls"] / 1e6}
        if shape is not None:
            row.update(M=shape[0], N=shape[1], K=shape[2], cfg=shape[3], k_slices=shape[4], gemm_kernels=shape[5])
        per_launch.append(row)
    per_launch.sort(key=lambda r: -r["us"] * r["calls_per_step"])
    streaming = [{"kernel": name, "rows": shape[0] if shape else None, "channels": shape[1] if shape else None,
                  "us": v["ms"] / v["calls"] * 1e3, "algorithmic_MB": v["bytes"] / v["calls"] / 1e6,
                  "GBps": v["bytes"] / v["ms"] / 1e6, "frac_of_achievable_hbm": v["bytes"] / v["ms"] / 1e6 / ACHIEVABLE_HBM_GBPS}
                 for (name, shape), v in streams.items()]
    streaming.sort(key=lambda r: -r["us"])
    dom = max(kernels, key=lambda k: kernels[k]["ms_per_step"])
    alg = kernels[dom]["tflops"]
    traffic, traffic_note = pmc_traffic(dom, math)
    by_kernel = None
    if math == "f16x3":
        # The DOMINANT KERNEL of the step: the launches grouped by the kernel that served them (tile configuration), not by
        # GEMM form -- one template serves forward and dgrad launches alike
        names = {22: "k_nt_s16<Cfg<2,4,4,2,2,32,0,1>> (256x256 tile, 8 waves of 128x64; forward + dgrad launches)",
                 28: "k_nt_s16<Cfg<2,4,4,2,2,32,0,1,3>> (224x256 tile, 8 waves: wave rows of 4 + 3 row blocks; the forward and "
                     "plain-dgrad launches of the 27,648-row layers: 496 / 1488 tiles = 1.94 / 5.81 rounds of 256 CUs)",
                 29: "k_nt_s16<Cfg<2,4,3,2,2,32,0,1,2>> (160x256 tile, 8 waves: wave rows of 3 + 2 row blocks; the 9,216-row launches: "
                     "232 tiles = 91 % of one round of 256 CUs; 3072 x 1024 x 3072 as 80 tiles x 3 K slices)",
                 1028: "k_nt_s16<Cfg<2,4,4,2,2,32,0,1,3>, RED> (224x256 tile dgrad + the BatchNorm-backward column sums of the upstream "
                       "activation, vp3d_s16_red)",
                 20: "k_nt_s16<Cfg<2,2,2,2,2,32,0,1>> (128x128 tile, 4 waves, 2 workgroups per CU)",
                 1022: "k_nt_s16<Cfg<2,4,4,2,2,32,0,1>, RED> (256x256 tile dgrad + the BatchNorm-backward column sums of the "
                       "upstream activation: reads that activation's conv output and bits in the epilogue, vp3d_s16_red)",
                 1020: "k_nt_s16<Cfg<2,2,2,2,2,32,0,1>, RED> (128x128 tile dgrad + BatchNorm-backward column sums)",
                 "tn": "k_tn_s16<2> (rows-form weight gradient, 256x256 tile, transpose reads)",
                 "ex": "k_expand_fwd_s16 (expand layer forward: statistics + activation pass)",
                 "exb": "k_expand_bwd_p_s16 (expand layer backward: P = G^T X from go + bits)",
                 None: "k_rows_gemm / k_red_gemm (fp32 MFMA kernels: the shrink conv's forward, dgrad and wgrad)"}
        grp = {}
        for r in per_launch:
            g = grp.setdefault(r.get("cfg"), dict(us=0.0, flops=0.0, mb=0.0, n=0.0))
            g["us"] += r["us"] * r["calls_per_step"]
            g["flops"] += r["tflops"] * r["us"] * r["calls_per_step"]        # TFLOP/s x us = MFLOP
            g["mb"] += r["algorithmic_MB"] * r["calls_per_step"]
            g["n"] += r["calls_per_step"]
        by_kernel = {str(names.get(k, k)): dict(launches_per_step=v["n"], us_per_step=v["us"], tflops=v["flops"] / v["us"],
                                                 frac_of_peak=v["flops"] / v["us"] / peak_alg,
                                                 algorithmic_MB_per_launch=v["mb"] / v["n"])
                     for k, v in grp.items() if v["us"] > 0}
        kdom = max(grp, key=lambda k: grp[k]["us"])
        kname = str(names.get(kdom, kdom))
        alg = grp[kdom]["flops"] / grp[kdom]["us"]
        live = [(r["M"], r["N"], r["K"], r["k_slices"]) for r in per_launch if r.get("cfg") == kdom
                for _ in range(int(round(r["calls_per_step"])))]
        traffic, traffic_note = pmc_traffic_of_cfg(kdom, math, live)          # None + the reason when the table is stale
        kernels[dom] = dict(kernels[dom])
        dom_launch = dict(calls_per_step=grp[kdom]["n"], avg_launch_ms=grp[kdom]["us"] / grp[kdom]["n"] / 1e3,
                          algorithmic_bytes_per_launch=grp[kdom]["mb"] / grp[kdom]["n"] * 1e6)
        peak = PEAK_F16_MFMA_TFLOPS / MFMA_PER_MAC_F16X3
        extra = {"executed_mfma_tflops": alg * MFMA_PER_MAC_F16X3, "mfma_peak_f16_dense": PEAK_F16_MFMA_TFLOPS,
                 "sustained_mfma_f16_random_operands": SUSTAINED_F16_MFMA_TFLOPS,
                 "frac_of_sustained_mfma": alg * MFMA_PER_MAC_F16X3 / SUSTAINED_F16_MFMA_TFLOPS,
                 "frac_of_fp32_mfma_peak": alg / PEAK_F32_MFMA_TFLOPS,
                 "note": "split-fp16 GEMM: every algorithmic MAC is 3 f16 MFMA MACs (ah*bh + ah*bl + al*bh), so peak = "
                         "2500 / 3 TFLOP/s of algorithmic work; achieved = sum of algorithmic conv FLOPs (2*M*N*K) of the "
                         "dominant kernel's launches / sum of their HIP-event durations on the launch stream (`kernels` holds "
                         "the same per GEMM form, `by_kernel` per kernel); frac = executed MFMA "
                         "FLOP/s / dense f16 MFMA peak (nominal, 2.4 GHz); frac_of_sustained_mfma = the same against what a bare "
                         "MFMA loop sustains on random operands under this chip's power management (tools/ubench/mfma_peak.hip).  "
                         "frac_of_fp32_mfma_peak > 1 means faster than the exact-fp32 MFMA path could run at 100 % of its roofline"}
    else:
        kname = {"tconv_fwd": "k_rows_gemm<true,*> (vp3d_tconv_fwd)", "tconv_dgrad": "k_rows_gemm<false,*> (vp3d_tconv_dgrad)",
                 "tconv_wgrad": "k_red_gemm<*> (vp3d_tconv_wgrad)"}[dom]
        peak = PEAK_F32_MFMA_TFLOPS
        extra = {"note": "achieved = sum of algorithmic conv FLOPs (2*M*N*K) of the family's launches / sum of their "
                         "HIP-event durations on the launch stream"}
    dl = dom_launch if math == "f16x3" else kernels[dom]
    roof = {"bound": "mfma", "achieved": alg, "peak": peak, "unit": "TFLOP/s", "frac": alg / peak,
            "traffic": traffic, "traffic_note": traffic_note,
            "algorithmic_bytes": dl["algorithmic_bytes_per_launch"], "kernel": kname,
            "launches_per_step": dl["calls_per_step"], "avg_launch_ms": dl["avg_launch_ms"]}
    roof.update(extra)
    if by_kernel is not None:
        roof["by_kernel"] = by_kernel            # every GEMM kernel of the step: time, algorithmic TFLOP/s, fraction of the roofline
    roof["per_launch"] = per_launch          # one row per distinct GEMM launch of the step (what profiles/r04_step_table.txt shows
    roof["streaming"] = streaming[:6]        # from rocprofv3); the two big HBM-bound producers against the achievable HBM rate
    return roof, kernels


def dropin_steps(dev, x, tgt, math, headline_ms):
    """What an UNEDITED run.py gets from this package: only `from common.model import *` (run.py:21) resolves to the shim
    (videopose3d_amd/common/model.py); everything else is the reference's own loop, run.py:401-420, restated line by line:
    torch `mean(norm(pred - target))` (common/loss.py:11-17, ~10 torch kernels + autograd), `optimizer.zero_grad()`, autograd's
    `.grad` accumulation through the module boundary, `loss.item()` (run.py:414: a host synchronisation EVERY step -- the queue
    drains, the next step's launches start from an idle GPU) and `torch.optim.Adam(amsgrad=True).step()` (run.py:252,420).
    `dropin_step`: batches already on the device.  `dropin_step_with_h2d`: additionally run.py:402-407 -- a float64 numpy
    batch (what the reference's ChunkedGenerator yields) -> astype('float32') -> from_numpy -> .cuda() (pageable host memory),
    root joint zeroed.  The reference generator's own Python batch assembly (generators.py:105-149) is NOT in either number.
    The headline (`value`) and `full_step` use three opt-in edits instead: the fused loss (vp3d_mpjpe), gradients written
    straight into the flat exchange buffer (dp.FlatGradSync) and, for full_step, the device generator + fused Adam."""
    import importlib
    pkg_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "videopose3d_amd")
    sys.path.insert(0, pkg_dir)                      # the shim directory ahead of everything, as INTEGRATION.md prescribes
    try:
        shim = importlib.import_module("common.model")
    finally:
        sys.path.remove(pkg_dir)
    torch.manual_seed(0)
    model = shim.TemporalModelOptimized1f(17, 2, 17, FW, causal=False, dropout=0.25, channels=C)
    model = model.cuda()                             # run.py:250-251
    model.math = math
    model.train()                                    # run.py:318
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3, amsgrad=True)      # run.py:252

    def ref_mpjpe(predicted, target):                # common/loss.py:11-17
        assert predicted.shape == target.shape
        return torch.mean(torch.norm(predicted - target, dim=len(target.shape) - 1))

    acc = [0.0]

    def step_dev(inputs_2d=x, inputs_3d=tgt):
        optimizer.zero_grad()
        predicted_3d_pos = model(inputs_2d)
        loss_3d_pos = ref_mpjpe(predicted_3d_pos, inputs_3d)
        acc[0] += inputs_3d.shape[0] * inputs_3d.shape[1] * loss_3d_pos.item()
        loss_3d_pos.backward()
        optimizer.step()

    batch_2d = x.detach().cpu().numpy().astype(np.float64)        # generators.py:52-55: float64 buffers
    batch_3d = tgt.detach().cpu().numpy().astype(np.float64)

    def step_h2d():
        inputs_3d = torch.from_numpy(batch_3d.astype('float32'))
        inputs_2d = torch.from_numpy(batch_2d.astype('float32'))
        inputs_3d = inputs_3d.cuda()
        inputs_2d = inputs_2d.cuda()
        inputs_3d[:, :, 0] = 0
        step_dev(inputs_2d, inputs_3d)

    def timed(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ws = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            ws.append((time.perf_counter() - t0) / n * 1e3)
        return sorted(ws)[1], ws

    ms_a, ws_a = timed(step_dev, 10)
    ms_b, ws_b = timed(step_h2d, 5)
    # where the difference to the headline goes: the same module call with the loss.item() synchronisation removed, and the
    # optimizer alone
    def step_nosync():
        optimizer.zero_grad()
        ref_mpjpe(model(x), tgt).backward()
        optimizer.step()
    ms_c, _ = timed(step_nosync, 10)
    del optimizer, model
    torch.cuda.empty_cache()
    a = {"what": "unedited run.py:408-420 behind the import shim: torch mpjpe + optimizer.zero_grad() + autograd .grad + loss.item() "
                 "+ torch.optim.Adam(amsgrad).step(); batch resident on the device", "ms": ms_a, "frames_per_s": B / ms_a * 1e3,
         "windows_ms": [round(v, 4) for v in ws_a], "ms_without_item_sync": ms_c}
    b = {"what": "the same + run.py:402-407: float64 numpy batch -> astype(float32) -> from_numpy -> .cuda() (pageable), root joint "
                 "zeroed", "ms": ms_b, "frames_per_s": B / ms_b * 1e3, "windows_ms": [round(v, 4) for v in ws_b]}
    return a, b, {"headline_ms": headline_ms, "dropin_over_headline": ms_a / headline_ms,
                  "note": "headline = fwd + bwd only (optimizer outside, reported as adam_ms / adam_torch_ms); dropin_step includes "
                          "torch Adam and the per-step loss.item() of run.py:414"}


def shape_sweep(dev, steps=20):
    """The reference's OWN default configuration and its neighbour (run.py defaults: `-arc 3,3,3 -b 1024`, reference
    common/arguments.py:37,45; and arc 3,3,3,3) at C = 1024: training step on both engines, eager and as a hipGraph replay.
    36.4 / 109 GFLOP of forward work per call sit either side of engine.S16_MIN_FORWARD_FLOPS (40 GFLOP): the table says which
    engine each lands on by default and what the other one would have cost."""
    import videopose3d_amd as V
    from videopose3d_amd import TemporalModelOptimized1f, dp, engine
    from videopose3d_amd import loss as vloss
    from videopose3d_amd.graph import GraphedTrainStep
    rows = []
    keep = dict(engine.S16_MIN_FORWARD_FLOPS)
    for fw in ([3, 3, 3], [3, 3, 3, 3]):
        rf = 1
        for f in fw:
            rf *= f
        g = torch.Generator().manual_seed(4321)
        xs = (torch.randn(B, rf, 17, 2, generator=g) * 0.5).clamp(-1, 1).to(dev)
        ts = (torch.randn(B, 1, 17, 3, generator=g) * 0.3).to(dev)
        row = {"arc": ",".join(map(str, fw)), "batch": B, "channels": C, "receptive_field": rf}
        for mth in ("f32", "f16x3"):
            torch.manual_seed(0)
            m = TemporalModelOptimized1f(17, 2, 17, fw, causal=False, dropout=0.25, channels=C).to(dev).train()
            m.math = mth
            row["forward_gflop"] = m._plan.forward_flops(B, rf) / 1e9
            row["default_engine"] = "f16x3" if m._plan.forward_flops(B, rf) >= keep[True] else "f32"
            engine.S16_MIN_FORWARD_FLOPS.update({True: 0.0, False: 0.0})     # f16x3 rows: the split-fp16 engine whatever the size
            try:
                sync = dp.FlatGradSync(m.parameters(), world=1, direct_module=m)

                def step():
                    sync.zero_grad()
                    vloss.mpjpe(m(xs), ts).backward()
                    sync.sync()

                def timed(fn):
                    for _ in range(5):
                        fn()
                    torch.cuda.synchronize()
                    best = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        for _ in range(steps):
                            fn()
                        torch.cuda.synchronize()
                        best.append((time.perf_counter() - t0) / steps * 1e3)
                    return sorted(best)[1]
                row[mth + "_eager_ms"] = timed(step)
                try:
                    gs = GraphedTrainStep(m, sync)
                    row[mth + "_replay_ms"] = timed(lambda: gs(xs, ts))
                    del gs
                except Exception as e:  # noqa: BLE001
                    row[mth + "_replay_error"] = repr(e)[:160]
            finally:
                engine.S16_MIN_FORWARD_FLOPS.update(keep)
            del m, sync
            torch.cuda.empty_cache()
        row["faster_eager"] = "f16x3" if row["f16x3_eager_ms"] < row["f32_eager_ms"] else "f32"
        rows.append(row)
    return {"what": "train step fwd+bwd (dropout 0.25) at B=1024, C=1024 for run.py's default arc 3,3,3 and for 3,3,3,3: both "
                    "engines, eager module call and hipGraph replay; default_engine = what engine.S16_MIN_FORWARD_FLOPS "
                    "(%.0f GFLOP of forward work) selects" % (keep[True] / 1e9), "rows": rows}


DUMP_MAX_ELEMS = 1 << 20


def dump_outputs(out_dir, loss, pred, model):
    """--dump-outputs: what the caller of the timed step receives from its last execution, as float32 .npy files (loss, predicted
    poses, every parameter's gradient).  A gradient above DUMP_MAX_ELEMS elements is written as the same seeded sample of its
    flattened values in every run (at most ~40 MB in all for the benchmark model), so that two builds compare file for file."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss": loss, "pred": pred}
    arrays.update(("grad." + n, p.grad) for n, p in model.named_parameters())
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if a.size > DUMP_MAX_ELEMS:
            idx = np.sort(np.random.default_rng(0).choice(a.size, DUMP_MAX_ELEMS, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def relaunch_under_torchrun(n_gpus):
    """`python bench.py --gpus N` without an external launcher: start N ranks of this script through
    torch.distributed.run on one node (rendezvous on 127.0.0.1, a free port) and hand back its exit code; rank 0 of the
    children prints the ONE JSON line on the inherited stdout.  Under an external launcher (WORLD_SIZE set: the driver's
    `python -m torch.distributed.run ... bench.py --gpus N`) this is never reached."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: what RCCL needs between the ranks of one node
    env.setdefault("OMP_NUM_THREADS", "1")                  # N python ranks share the host's cores: no oneDNN/OpenMP pools
    from videopose3d_amd import dp
    for k, v in dp.RCCL_ENV_DEFAULTS.items():               # RCCL's channel budget beside the backward GEMMs (dp.py; also set by
        env.setdefault(k, v)                                # dp.init_from_env under an external launcher: the driver's torchrun)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def dry_run(args):
    """--dry-run: the distributed control flow of the benchmark without any GPU work (CPU test of the launcher and of
    the barrier / max-over-ranks timing contract): rendezvous (gloo), W + K empty steps between barriers, rank 0 prints
    the JSON skeleton with value null."""
    from videopose3d_amd import dp
    rank, world, local = dp.init_from_env("gloo")
    assert world == args.gpus, (world, args.gpus)
    cores = dp.pin_rank_to_cores(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    if world > 1:
        allc = [None] * world
        dist.all_gather_object(allc, cores)
    else:
        allc = [cores]
    for _ in range(args.warmup):
        pass
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pass
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        out = {"metric": "frames/sec (fwd+bwd) 243-frame arc=3,3,3,3,3 B=1024", "value": None, "unit": "frames/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": None,
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dry_run": True,
               "barrier_to_barrier_s": dt,
               "launcher": {"rccl_env": {k: os.environ.get(k) for k in dp.RCCL_ENV_DEFAULTS} if world > 1 else None,
                            "cores_per_rank": allc}}
        if os.environ.get("VP3D_DRY_RUN_DETAIL"):        # CPU test hook: a full-size record (e.g. the committed r04 line) through
            with open(os.environ["VP3D_DRY_RUN_DETAIL"]) as f:      # the SAME final_line() the GPU run prints
                big = json.load(f)
            big.update(out)
            out = big
        print(final_line(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=1, help="timed windows of --steps steps each (default: one, so that --steps is "
                    "the number of timed steps); `value` is the median window")
    ap.add_argument("--no-settle", action="store_true", help="skip the untimed settle phase before the warm-up")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-eval", action="store_true", help="skip the cfg2 eval-forward section")
    ap.add_argument("--no-f32", action="store_true", help="skip the exact-fp32 MFMA comparison sections")
    ap.add_argument("--math", default=None, help="arithmetic of the headline: f16x3 (default) or f32")
    ap.add_argument("--no-rocm-ref", action="store_true", help="skip the PyTorch-ROCm (MIOpen) reference-path baseline (~75 s)")
    ap.add_argument("--no-sweep", action="store_true", help="skip the shape sweep (run.py's default arc 3,3,3 / 3,3,3,3 on both engines)")
    ap.add_argument("--dry-run", action="store_true", help="launcher / barrier control flow only, no GPU work (CPU test hook)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (loss, predicted poses, parameter gradients; "
                         "a fixed seeded sample of each gradient above %d elements) to DIR/<name>.npy" % DUMP_MAX_ELEMS)
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch_under_torchrun(args.gpus))       # bare `python bench.py --gpus N`: one rank per GPU, ourselves
    if args.dry_run:
        return dry_run(args)

    import videopose3d_amd as V
    from videopose3d_amd import TemporalModel, TemporalModelOptimized1f, dp, ops
    from videopose3d_amd import loss as vloss
    # VP3D_DIST_BACKEND / VP3D_BENCH_DEVICE are test hooks: "gloo" + device 0 let the N > 1 control flow (matched
    # collectives on every rank, no deadlock) be exercised on a box with a single GPU; the driver never sets them.
    rank, world, local = dp.init_from_env(os.environ.get("VP3D_DIST_BACKEND", "nccl"))
    assert world == args.gpus, "WORLD_SIZE=%d but --gpus %d: launch one rank per GPU" % (world, args.gpus)
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP path has no CPU fallback)"
    pinned = dp.pin_rank_to_cores(local, int(os.environ.get("LOCAL_WORLD_SIZE", world))) if world > 1 else None
    local = int(os.environ.get("VP3D_BENCH_DEVICE", local))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    math = args.math or V.default_math()

    gen = torch.Generator().manual_seed(1234 + rank)
    x, tgt = synthetic_batch(B, gen)
    x, tgt = x.to(dev), tgt.to(dev)                      # inputs resident in HBM before the timed region

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def build(mth):
        torch.manual_seed(0)
        model = TemporalModelOptimized1f(17, 2, 17, FW, causal=False, dropout=0.25, channels=C).to(dev).train()
        model.math = mth
        sync = dp.FlatGradSync(model.parameters(), world=world, direct_module=model)
        sync.broadcast_parameters(model.buffers())

        def step():
            sync.zero_grad()
            pred = model(x)
            loss = vloss.mpjpe(pred, tgt)               # loss.py:11-17 on the HIP path (one kernel: value + gradient)
            loss.backward()
            sync.sync()
            last["pred"], last["loss"] = pred.detach(), loss.detach()
            return loss
        return model, sync, step
    last = {}

    def one_window(step, steps, events=True):
        """EXACTLY `steps` steps between two fences (barrier + device sync on both sides), max over ranks.  Also returned:
        the host's enqueue time for the window (loop end, before the closing fence) and, with `events`, the GPU-side duration
        of every step (HIP events recorded on the launch stream between the steps: the backward of a step joins the second
        stream before it returns, so consecutive events bracket a whole step)."""
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)] if events else None
        fence()
        t0 = time.perf_counter()
        for i in range(steps):
            if events:
                evs[i].record()
            step()
        if events:
            evs[steps].record()
        t_host = time.perf_counter() - t0
        fence()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt, t_host], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt, t_host = float(t[0].item()), float(t[1].item())
        per_step = [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)] if events else None
        return dt, t_host, per_step

    def settle(step, steps, tol=0.02, max_windows=12):
        """Untimed settle phase BEFORE the official warm-up: windows of `steps` steps (the shape of the timed windows, so the
        host's run-ahead and with it the caching allocator's high-water mark are the timed region's) until two consecutive
        windows agree within `tol` -- a fresh process on a fresh lease needs that long for its clocks / power state, the
        allocator's pools on both streams and the lazily loaded code objects to stop moving (BENCH_r02: the first 0.12 s
        window after 5 warm-up steps measured 5.997 ms / step, the same process 4.76 ms a minute later)."""
        ms = []
        while len(ms) < max_windows:
            dt, _, _ = one_window(step, steps, events=False)
            ms.append(dt / steps * 1e3)
            if len(ms) >= 2 and abs(ms[-1] - ms[-2]) <= tol * min(ms[-1], ms[-2]):
                break
        # every rank must leave after the same number of windows (the windows hold collectives): dt is already the max over ranks
        return ms

    def time_steps(step, warmup, steps, windows=1, do_settle=False, detail=None, model=None):
        """W untimed warm-up steps, then `windows` timed windows of EXACTLY `steps` steps each; the reported time is the
        MEDIAN window (all windows are listed in `detail`)."""
        settle_ms = settle(step, steps) if do_settle else []
        if model is not None:
            model._drop_calls = 0          # the dropout masks of warm-up and timed steps do not depend on how long settle ran
        for _ in range(warmup):
            step()
        res = [one_window(step, steps, events=detail is not None) for _ in range(windows)]
        order = sorted(range(windows), key=lambda i: res[i][0])
        mid = order[(windows - 1) // 2]                      # (lower) median window
        if detail is not None:
            detail.update(settle_windows=len(settle_ms), settle_ms_per_step=[round(v, 4) for v in settle_ms],
                          windows_ms_per_step=[round(r[0] / steps * 1e3, 4) for r in res], median_window=mid,
                          step_ms=[round(v, 4) for v in res[mid][2]],
                          host_ms_per_step=res[mid][1] / steps * 1e3,
                          step_ms_all_windows_max=max(max(r[2]) for r in res), step_ms_all_windows_min=min(min(r[2]) for r in res))
        return res[mid][0]

    n_windows = max(1, args.windows)
    model, sync, step = build(math)
    timing = {}
    dt = time_steps(step, args.warmup, args.steps, windows=n_windows, do_settle=not args.no_settle, detail=timing, model=model)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last["loss"], last["pred"], model)
    last.clear()
    ms_per_step = dt / args.steps * 1e3
    value = world * B * args.steps / dt
    dtype = "f16x3 (split-fp16 operands, fp32 accumulate)" if math == "f16x3" else "f32"

    out = {
        "metric": "frames/sec (fwd+bwd) 243-frame arc=3,3,3,3,3 B=1024", "value": value, "unit": "frames/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype, "math": math, "data": "synthetic",
        "config": {"workload": "cfg3: TemporalModelOptimized1f train step fwd+bwd (BN stats, dropout 0.25), "
                               "arc 3,3,3,3,3 C=1024, per-GPU B=1024 x 243 frames x 17 joints",
                   "global_batch": world * B, "parallelism": "dp%d" % world,
                   "grad_allreduce_bytes": sync.numel * 4 if world > 1 else 0},
        "step_tflops": FLOP_TRAIN_PER_FRAME * value / 1e12,
        "step_frac_of_fp32_mfma_peak": FLOP_TRAIN_PER_FRAME * value / 1e12 / (PEAK_F32_MFMA_TFLOPS * world),
        "step_frac_of_roofline": FLOP_TRAIN_PER_FRAME * value / 1e12 / world /
        (PEAK_F16_MFMA_TFLOPS / MFMA_PER_MAC_F16X3 if math == "f16x3" else PEAK_F32_MFMA_TFLOPS),
        # how `value` was timed: an untimed settle phase (windows of --steps steps until two consecutive ones agree within
        # 2 %), --warmup steps, then --windows windows of EXACTLY --steps steps, each between barrier + device-sync fences;
        # value = the median window.  step_ms = HIP-event duration of every step of that window; host_ms_per_step = the
        # host's enqueue time per step in it (Python + ctypes with the GPU running behind: host-bound when it reaches ms_per_step)
        "timing": dict(timing, windows=n_windows, value_is="median window",
                       host_bound=bool(timing["host_ms_per_step"] >= 0.9 * ms_per_step)),
    }

    # ---- the same step replayed as ONE hipGraph (graph.GraphedTrainStep: forward + fused mpjpe + backward captured once;
    # the batch, the BatchNorm running statistics and the dropout step counter live in device memory).  The eager module
    # call above is the drop-in for run.py and stays `value`; the replay removes the host's launch gaps (the T_out = 1..9
    # tail of backward is host-bound in eager mode).
    if os.environ.get("VP3D_BENCH_GRAPH", "1") == "1":
        try:
            from videopose3d_amd.graph import GraphedTrainStep
            gstep = GraphedTrainStep(model, sync)
            gdetail = {}
            dt_g = time_steps(lambda: gstep(x, tgt), 3, args.steps, windows=min(3, n_windows), detail=gdetail)
            out["graph_replay"] = {"what": "the same step (same model, batch, dropout 0.25, gradient sink) replayed from hipGraphs "
                                           "(videopose3d_amd.graph.GraphedTrainStep: graph pieces per stream, so that the two-stream "
                                           "overlap of backward survives -- one graph replays its branches serially on this runtime); "
                                           "the gradient exchange for N > 1 follows the replay", "ms_per_step": dt_g / args.steps * 1e3,
                                   "frames_per_s": world * B * args.steps / dt_g, "speedup_vs_eager": dt / dt_g,
                                   "windows_ms_per_step": gdetail["windows_ms_per_step"],
                                   "host_ms_per_step": gdetail["host_ms_per_step"]}
            del gstep
        except Exception as e:  # noqa: BLE001  (informational: never lets the headline line fail)
            out["graph_replay"] = {"error": "%s: %s" % (type(e).__name__, e)}

    # N > 1: the host side counts (N Python ranks enqueue ~2 ms of launches per 4.4 ms step each on the node's cores): both forms of
    # the SAME step were timed above -- eager and hipGraph pieces -- and `value` is the faster one; `value_path` says which, the
    # other stays in `eager` / `graph_replay`.  One GPU: `value` is always the eager module call (the drop-in for run.py).
    out["value_path"] = "eager"
    out["launcher"] = {"rccl_env": {k: os.environ.get(k) for k in dp.RCCL_ENV_DEFAULTS} if world > 1 else None,
                       "cores_of_rank0": pinned}
    gr = out.get("graph_replay", {})
    if world > 1 and gr.get("ms_per_step") and gr["ms_per_step"] < ms_per_step:
        out["eager"] = {"value": value, "ms_per_step": ms_per_step}
        out["value_path"] = "graph_replay"
        value, ms_per_step = gr["frames_per_s"], gr["ms_per_step"]
        out["value"], out["ms_per_step"] = value, ms_per_step
        out["step_tflops"] = FLOP_TRAIN_PER_FRAME * value / 1e12
        out["step_frac_of_fp32_mfma_peak"] = out["step_tflops"] / (PEAK_F32_MFMA_TFLOPS * world)
        out["step_frac_of_roofline"] = out["step_tflops"] / world / (PEAK_F16_MFMA_TFLOPS / MFMA_PER_MAC_F16X3 if math == "f16x3"
                                                                     else PEAK_F32_MFMA_TFLOPS)

    # Everything below that runs training steps is executed by EVERY rank: a step contains collectives (the bucketed
    # all-reduces launched from inside backward and the final wait), so a rank-0-only step would deadlock for N > 1.
    # Kernel launches of one eager step: the library counts its own (vp3d_launch_count); torch adds the flat buffer's zero_() and
    # the three elementwise kernels of loss.backward() (ones_like, grad * gout, the view's copy) -- the step is ONE dependent chain,
    # so the count is a lever of its own (round 5: ~0.5 us of argument fetch per launch before device kernargs)
    from videopose3d_amd import _lib as _vl
    n0_l = _vl.lib().vp3d_launch_count()
    step()
    torch.cuda.synchronize()
    out["launches_per_step"] = {"libvp3d": int(_vl.lib().vp3d_launch_count() - n0_l), "torch_elementwise": 4}
    out["roofline"], out["kernels"] = instrumented(step, ops, 3, math)
    from videopose3d_amd import range_guard
    out["range_guard"] = {k: v for k, v in range_guard.status(model).items() if k in ("tripped", "last", "io_last", "checks", "gram_off", "gram_log2_kappa")}
    out["range_guard"]["tick_us_per_call"] = round(range_guard.status(model).get("tick_us_per_call", 0.0), 1)
    if world == 1:
        try:
            out["box"] = box_state(step, local)
        except Exception as e:  # noqa: BLE001  (diagnostics never cost the run its result)
            out["box"] = {"error": repr(e)[:200]}
    gemm_ms = sum(v["ms_per_step"] for v in out["kernels"].values())
    out["non_gemm_ms_per_step"] = ms_per_step - gemm_ms if world == 1 else None

    # ---- the callers either side of the stack, outside the metric -------------------------
    def timed(fn, n=5):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    opt = torch.optim.Adam(model.parameters(), lr=1e-3, amsgrad=True)      # run.py:252,264
    out["adam_torch_ms"] = timed(opt.step)
    del opt
    from videopose3d_amd.optim import FlatAdam
    from videopose3d_amd.generators import ChunkedGenerator
    fopt = FlatAdam(model.parameters(), lr=1e-3, amsgrad=True, grad_sync=sync)
    out["adam_ms"] = timed(fopt.step)                                       # vp3d_adam_step, one pass
    rng = np.random.RandomState(0)
    lens = [3000 + 517 * i for i in range(24)]                              # ~216k frames of synthetic "videos"
    p2 = [rng.standard_normal((n, 17, 2)).astype(np.float32) for n in lens]
    p3 = [rng.standard_normal((n, 17, 3)).astype(np.float32) for n in lens]
    gen_dev = ChunkedGenerator(B, None, p3, p2, 1, pad=(RF - 1) // 2, shuffle=True, augment=True,
                               kps_left=[1, 3, 5, 7, 9, 11, 13, 15], kps_right=[2, 4, 6, 8, 10, 12, 14, 16],
                               joints_left=[4, 5, 6, 11, 12, 13], joints_right=[1, 2, 3, 14, 15, 16], device=dev)
    it = gen_dev.next_epoch()
    out["batch_gather_ms"] = timed(lambda: next(it), n=10)                  # vp3d_gather_chunks, B=1024 x 243 frames

    def full_step():
        _, b3, b2 = next(it)
        b3[:, :, 0] = 0                                                     # run.py:407
        fopt.zero_grad()
        vloss.mpjpe(model(b2), b3).backward()
        sync.sync()                                                         # no-op for one GPU
        fopt.step()
    ms_full = timed(full_step, n=10)
    out["full_step"] = {"what": "device batch assembly + fwd + bwd + fused Adam (run.py:401-420 end to end), B=1024",
                        "ms": ms_full, "frames_per_s": B / ms_full * 1e3}
    # full_step is a strict superset of the headline step: a headline slower than 1.1 x it was hit by something outside the
    # step (clock / power state, allocator growth, another process on the box) -- look at timing.step_ms / windows_ms_per_step
    out["headline_suspect"] = bool(world == 1 and ms_per_step > 1.1 * ms_full)

    # ---- the path run.py actually gets with NO edit but the import shim (world 1 only: torch.optim has no gradient exchange)
    if world == 1:
        out["dropin_step"], out["dropin_step_with_h2d"], out["dropin_vs_headline"] = dropin_steps(dev, x, tgt, math, ms_per_step)
    del fopt, gen_dev, it, model, sync, step
    torch.cuda.empty_cache()

    # ---- the same step on the exact-fp32 MFMA kernels (every rank: the step holds collectives) -------------
    if math != "f32" and not args.no_f32:
        model, sync, step = build("f32")
        k32 = max(5, args.steps // 2)
        dt32 = time_steps(step, 3, k32, windows=min(3, n_windows))
        v32 = world * B * k32 / dt32
        roof32, kern32 = instrumented(step, ops, 3, "f32")
        out["f32_mfma"] = {"what": "the same training step with math='f32' (v_mfma_f32_32x32x2_f32, exact fp32 products)",
                           "value": v32, "unit": "frames/s", "ms_per_step": dt32 / k32 * 1e3, "steps": k32,
                           "step_tflops": FLOP_TRAIN_PER_FRAME * v32 / 1e12,
                           "step_frac_of_fp32_mfma_peak": FLOP_TRAIN_PER_FRAME * v32 / 1e12 / (PEAK_F32_MFMA_TFLOPS * world),
                           "roofline": roof32, "kernels": kern32}
        out["speedup_vs_f32_mfma"] = value / v32
        del model, sync, step
        torch.cuda.empty_cache()

    if rank == 0 and not args.no_eval:
        # ---- BASELINE.json configs[1]: dense eval forward, B=1024, T=243 ------------------------------
        def eval_section(mth):
            torch.manual_seed(0)
            ev = TemporalModel(17, 2, 17, FW, channels=C).to(dev).eval()
            ev.math = mth
            k_eval = max(3, args.steps // 4)
            with torch.no_grad():
                for _ in range(2):
                    ev(x)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(k_eval):
                    y = ev(x)
                torch.cuda.synchronize()
                dte = (time.perf_counter() - t0) / k_eval
                runs = []
                for _ in range(3):                     # per-launch rates: the median of three instrumented forwards
                    recs = []
                    ops.set_profiler(recs)
                    ev(x)
                    torch.cuda.synchronize()
                    ops.set_profiler(None)
                    runs.append([(f, e0.elapsed_time(e1)) for _, f, e0, e1, _b, _s in recs if f > 1e11])
            big = [(runs[0][i][0], sorted(r[i][1] for r in runs)[1]) for i in range(len(runs[0]))]
            tf = FLOP_EVAL_PER_FRAME * B / dte / 1e12
            return y, {"workload": "TemporalModel eval forward (BN folded), arc 3,3,3,3,3 C=1024 B=1024 T=243", "math": mth,
                       "ms": dte * 1e3, "frames_per_s": B / dte, "tflops": tf, "frac_of_fp32_mfma_peak": tf / PEAK_F32_MFMA_TFLOPS,
                       # fraction of THIS arithmetic's MFMA roofline (north_star: ">= 50 % ... TemporalModel forward at B=1024")
                       "frac": tf / (PEAK_F16_MFMA_TFLOPS / MFMA_PER_MAC_F16X3 if mth == "f16x3" else PEAK_F32_MFMA_TFLOPS),
                       "iters": k_eval, "big_gemm_tflops": [round(f / ms / 1e9, 1) for f, ms in big]}
        y_a, out["cfg2_eval_fwd"] = eval_section(math)
        if math != "f32" and not args.no_f32:
            y_b, out["cfg2_eval_fwd_f32_mfma"] = eval_section("f32")
            out["cfg2_eval_fwd"]["mpjpe_vs_f32_mfma"] = float(mpjpe(y_a, y_b))
            out["cfg2_eval_fwd"]["speedup_vs_f32_mfma"] = out["cfg2_eval_fwd_f32_mfma"]["ms"] / out["cfg2_eval_fwd"]["ms"]
            del y_b
        del y_a
        torch.cuda.empty_cache()

    if rank == 0 and world == 1:
        out["cfg5_semi_supervised_step"] = semi_supervised_step_latency(dev)
        if not args.no_sweep:
            try:
                out["shape_sweep"] = shape_sweep(dev)
            except Exception as ex:  # noqa: BLE001  (informational)
                out["shape_sweep"] = {"error": repr(ex)[:200]}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"], out["mpjpe_vs_ref"] = cpu_baseline(dev)
    if rank == 0 and world == 1 and not args.no_rocm_ref:
        try:
            ref = rocm_reference_baseline(dev, x, tgt)
            out["rocm_reference_baseline"] = ref
            out["speedup_vs_rocm_reference"] = value / ref["value"]
            if "cfg2_eval_fwd" in out:
                out["cfg2_eval_fwd"]["speedup_vs_rocm_reference"] = ref["cfg2_eval_ms"] / out["cfg2_eval_fwd"]["ms"]
        except Exception as ex:  # noqa: BLE001  (a missing MIOpen kernel database must not cost the run its result)
            out["rocm_reference_baseline"] = {"error": repr(ex)}

    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        out["detail_file"] = write_detail(out)
        print(final_line(out), flush=True)


if __name__ == "__main__":
    main()
