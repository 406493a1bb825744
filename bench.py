#!/usr/bin/env python
"""bench.py -- SiftPlan.keypoints() throughput on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2|c4] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the line: `value`, `ms_per_step`, the rooflines that the
timed steps themselves measure (or that are replayed from committed profiles).  Without the legs in front of it (below)
the GPU would enter the timed region from seconds of idle, on its clock ramp: a plain c2 run first repeats the headline
call for RAMP_S seconds, untimed, then runs the W warm-up steps.  `--full` adds everything else the benchmark measures:
the legs beside the headline (run first, N = 1: BatchPlan, host-to-host, keypoint-rich frame, MatchPlan 100k, C3 16384^2,
C4 on one GPU; at every N the 2-lane BatchPlan leg), `steady` (200 further steps) and the CPU baselines.
`--dump-outputs DIR` writes what the last timed step returned (dump_outputs) after the timed region.

`--gpus N` with N > 1 starts N ranks itself (one process per GPU, torch.distributed backend "nccl" = RCCL over xGMI)
unless it already runs under a launcher (WORLD_SIZE set, e.g. `python -m torch.distributed.run --nproc-per-node N
--master-addr 127.0.0.1 bench.py --gpus N ...`).  Rank 0 prints ONE JSON line.

config c2 (default, BASELINE.json configs[1]): a step = one SiftPlan.keypoints() over one 4096x4096 fp32 synthetic image
(uniform white noise) that is already resident in HBM when the timed region starts; 3 octaves x 3 scales.  With N > 1
each rank processes its own images -- independent units, no data-path collective ("weak" scaling) -- and the timed
region ends with the one exchange step of the batched path: an all-gather of the keypoint records of ALL K timed steps
(each step's records are kept in an arena in HBM by one device-to-device copy), from device memory (no host staging).

config c4 (BASELINE.json configs[3]): a step = one batch of 64 frames of 2048x2048 fp32, frame i owned by rank i mod N,
each rank's share pipelined through a BatchPlan, then the all-gather of EVERY frame's records on device tensors.  The
total work is fixed ("strong" scaling).

roofline: the dominant kernel family is the fused separable Gaussian blur (blur_team_kernel<N, NORM, S>).  Algorithmic
traffic = 1 read + 1 write of the plane = 8 B per pixel per launch; achieved = 6 * 8 * W*H / (hipEvent time
around the six full-resolution launches of an image: initial blur + the five scales of octave 0), measured live with
HIP events on the plan's own pyramid stream; those launches run alone on the GPU (the later octaves' launches overlap
the detection streams and cannot be timed in isolation).  roofline_pipeline is the whole-call figure of SURVEY 8d:
bytes_alg = W*H*(12 + 66*sum_o 4^-o) + 144 B/keypoint over the hipEvent time of all kernels of a call.

cpu_baseline: the CPU oracle (a port of the reference's OpenCL-CPU kernels, OpenMP over all host cores) timed on rank 0
on the same workload, and the reference's own kernels (built natively, one thread) -- reported baselines, not targets.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PROFILE_DIR = "profiles/r06"           # the round's rocprofv3 summaries (tools/collect_round.sh); replayed only for the library they describe


def library_fingerprint():
    from sift_pyocl_amd import _lib
    return _lib.source_fingerprint()


import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
SIZE = 4096
OCTAVES = 3
C4_FRAMES, C4_SIZE = 64, 2048
RAMP_S = 0.5            # untimed repeats of the headline call in a plain run: ~25 calls bring the clocks back (tools/dev/ramp.py)
DUMP_MAX_ROWS = 100000  # rows of 133 float32 each: a dump stays under 64 MB


def make_image(seed, size=SIZE):
    return np.random.default_rng(seed).random((size, size), dtype=np.float32)


def dump_outputs(path, frames_kp):
    """Write the keypoint records a caller received from the last timed step, frame by frame, as .npy files under `path`:
    keypoints.npy (n, 4) float32 x, y, scale, angle; descriptors.npy (n, 128) float32; frame.npy (n,) float32, the frame of
    each row; counts.npy (frames,) float64, the keypoints of each frame.  Within a frame the records are sorted by their
    bytes (the library's order is not specified); above DUMP_MAX_ROWS rows a fixed, seeded sample of rows is written."""
    parts, frame = [], []
    for f, k in enumerate(frames_kp):
        k = np.ascontiguousarray(k).view(np.uint8).reshape(len(k), 144)      # the 144-byte records
        key = np.lexsort(k.T[::-1])
        parts.append(k[key])
        frame.append(np.full(len(k), f, np.float32))
    rec = np.concatenate(parts) if parts else np.zeros((0, 144), np.uint8)
    frame = np.concatenate(frame) if frame else np.zeros(0, np.float32)
    if len(rec) > DUMP_MAX_ROWS:
        pick = np.sort(np.random.default_rng(0).choice(len(rec), DUMP_MAX_ROWS, replace=False))
        rec, frame = rec[pick], frame[pick]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "keypoints.npy"), np.ascontiguousarray(rec[:, :16]).view(np.float32))
    np.save(os.path.join(path, "descriptors.npy"), rec[:, 16:].astype(np.float32))
    np.save(os.path.join(path, "frame.npy"), frame)
    np.save(os.path.join(path, "counts.npy"), np.array([len(k) for k in frames_kp], np.float64))
    return len(rec)


def bytes_alg(w, h, n_oct, n_kp):
    return w * h * (12.0 + 66.0 * sum(4.0 ** -o for o in range(n_oct))) + 144.0 * n_kp


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            names = [line.split(":", 1)[1].strip() for line in f if line.startswith("model name")]
        return "%s (%d logical cpus)" % (names[0], len(names)) if names else "unknown"
    except Exception:
        return "unknown"


def cpu_baseline(size, octaves):
    """Oracle (port of the reference CPU kernels) on the host cores; bounded sample."""
    from oracle import pyoracle
    threads = os.cpu_count() or 1
    os.environ.setdefault("OMP_NUM_THREADS", str(threads))
    img = make_image(0, size)
    par = pyoracle.default_params(octave_max=octaves)
    pyoracle.keypoints(make_image(1, 512), par)          # load + thread pool warm-up
    t0 = time.perf_counter()
    reps = 0
    nkp = 0
    while True:
        k = pyoracle.keypoints(img, par)
        nkp = len(k)
        reps += 1
        el = time.perf_counter() - t0
        if el > 10.0 or reps >= 16:
            break
    mpix = reps * size * size / 1e6 / el
    return {"value": round(mpix, 3), "unit": "Mpix/s", "cores": threads, "kind": "port", "cpu": cpu_model(),
            "keypoints_per_s": round(reps * nkp / el, 1),
            "sample": "%d x SiftPlan-equivalent pass over one %dx%d fp32 white-noise image, %d octaves, "
                      "oracle/sift_oracle.c with OpenMP on %d threads (%.1f s wall)" % (reps, size, size, octaves, threads, el),
            "note": "a reported baseline, not a target: the port gains only ~10x from 256 threads over the reference's own kernels "
                    "on one thread (cpu_baseline_reference_kernels) -- memory-bound blurs, serial list handling"}


def cpu_reference_kernels(size, octaves):
    """The reference's OWN OpenCL-CPU kernels, compiled natively into oracle/_ref (when that build travelled with the
    snapshot), driven serially on one host thread over ONE pass of the same frame.  None if the library is absent."""
    try:
        from oracle import pyref
        if not pyref.available():
            return None
        img = make_image(0, size)
        pyref.keypoints(make_image(1, 256), octave_max=octaves)
        t0 = time.perf_counter()
        k = pyref.keypoints(img, octave_max=octaves)
        el = time.perf_counter() - t0
        return {"value": round(size * size / 1e6 / el, 3), "unit": "Mpix/s", "cores": 1, "kind": "reference",
                "keypoints_per_s": round(len(k) / el, 1),
                "sample": "1 pass of the reference's own kernels (openCL/*.cl built natively, oracle/_ref) over one %dx%d fp32 "
                          "white-noise image, %d octaves, serial NDRange on 1 thread (%.1f s wall)" % (size, size, octaves, el)}
    except Exception as exc:          # the baseline is a report, never a reason to lose the bench line
        return {"error": str(exc)[:200]}


def rank_envs(n, port, base=None):
    """The environment of each of the N ranks `--gpus N` starts on ONE node (what `torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1` would set): rank r is pinned to GPU r through LOCAL_RANK (main() calls
    torch.cuda.set_device(LOCAL_RANK); the plans take the same ordinal), one rendezvous port for all of them, dmabuf IPC
    for RCCL (HSA_ENABLE_IPC_MODE_LEGACY=0), one OpenMP thread per rank unless the caller set a count."""
    base = dict(os.environ if base is None else base)
    envs = []
    for r in range(n):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", "1")     # as torch.distributed.run does: N ranks must not each spin on every core
        envs.append(env)
    return envs


def spawn_ranks(args):
    """`--gpus N` without a launcher: start N copies of this script, one per GPU, and wait for them."""
    import torch
    visible = torch.cuda.device_count()
    if visible < 1:
        raise SystemExit("bench.py needs an MI355X: no HIP device is visible (there is no CPU fallback)")
    if args.gpus > visible and not args.share_gpu:
        raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible (use --share-gpu to rehearse the N>1 path on one GPU)"
                         % (args.gpus, visible))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r, env in enumerate(rank_envs(args.gpus, port)):
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    for p in procs:
        rc = p.wait() or rc
    raise SystemExit(rc)


# ---- VALU roofline (round 4).  Issue intervals per wave-instruction and SIMD, measured on this chip with
# tools/ubench/valu_rate.hip (profiles/r06/valu_issue_rate.txt; 8 waves per SIMD, 8 independent chains, shader clock read
# beside it): plain f32 add / mul / fma and u32 add / sub / logic / right shifts / v_mov 2.4 cycles; every other class
# (packed f32, f64, conversions, compares, selects, left shifts, 3-operand integer ops, DPP, mbcnt, v_sad) 4.2; f32
# transcendentals 8.2, f64 ones 16.2.  The hardware guide's "2 cycles per wave64 op" holds for the first class only.
VALU_SIMDS = 1024
VALU_CLOCK_GHZ = 2.3          # shader clock the ubench reads under VALU load (2.1-2.4)
VALU_CYCLES = {"f32": 2.4, "f32_packed": 4.2, "f64": 4.2, "trans_f32": 8.2, "trans_f64": 16.2, "cvt": 4.2, "int32": 3.3, "int64": 4.3, "other": 3.3}


def roofline_valu(ms_per_step):
    """Issue time of one headline frame's VALU instructions (committed PMC counts x measured issue intervals) against the
    measured time of a step.  `frac` = the share of a step during which every SIMD of the chip would have to issue VALU
    instructions back to back; the counts are replayed from the committed file, not observed in this run."""
    rel = PROFILE_DIR + "/valu_frame.json"
    try:
        vf = json.load(open(os.path.join(ROOT, rel)))
    except Exception:
        return None
    if vf.get("library_fingerprint") != library_fingerprint():
        # counts of other kernels than the ones loaded: not replayed (the summary has to be collected again: tools/valu_frame.sh)
        return {"bound": "valu", "achieved": None, "frac": None, "source": "%s was taken from a library with other sources (fingerprint %s, "
                "loaded %s): not replayed" % (rel, vf.get("library_fingerprint"), library_fingerprint())}
    cycles = 0.0
    instr = 0.0
    for fam, d in vf["families"].items():
        c = d["classes"]
        f32 = c["ADD_F32"] + c["MUL_F32"] + c["FMA_F32"]
        packed = fam.startswith("blur")          # the blur kernels do their arithmetic in v_pk_mul_f32 / v_pk_add_f32
        cycles += f32 * VALU_CYCLES["f32_packed" if packed else "f32"]
        cycles += (c["ADD_F64"] + c["MUL_F64"] + c["FMA_F64"]) * VALU_CYCLES["f64"]
        cycles += c["TRANS_F32"] * VALU_CYCLES["trans_f32"] + c["TRANS_F64"] * VALU_CYCLES["trans_f64"]
        cycles += c["CVT"] * VALU_CYCLES["cvt"] + c["INT32"] * VALU_CYCLES["int32"] + c["INT64"] * VALU_CYCLES["int64"]
        cycles += max(d["other"], 0.0) * VALU_CYCLES["other"]
        instr += d["valu"]
    if instr <= 0 or ms_per_step <= 0:
        return None
    issue_ms = cycles / (VALU_SIMDS * VALU_CLOCK_GHZ * 1e9) * 1e3
    mean_cycles = cycles / instr
    peak = VALU_SIMDS * VALU_CLOCK_GHZ / mean_cycles                   # G wave-instructions / s at this frame's class mix
    achieved = instr / 1e9 / (ms_per_step / 1e3)
    return {"bound": "valu", "achieved": round(achieved, 1), "peak": round(peak, 1), "unit": "G wave-instr/s", "frac": round(achieved / peak, 4),
            "instr_per_frame": round(instr), "mean_issue_cycles": round(mean_cycles, 2), "issue_ms_per_frame": round(issue_ms, 4),
            "issue_ms_if_all_full_rate": round(instr * 2.4 / (VALU_SIMDS * VALU_CLOCK_GHZ * 1e9) * 1e3, 4),
            "issue_ms_if_all_half_rate": round(instr * 4.2 / (VALU_SIMDS * VALU_CLOCK_GHZ * 1e9) * 1e3, 4),
            "simds": VALU_SIMDS, "clock_ghz": VALU_CLOCK_GHZ, "cycles_per_class": VALU_CYCLES,
            "source": "instruction counts replayed from %s (rocprofv3 --pmc SQ_INSTS_VALU* of this command, tools/valu_frame.sh); "
                      "issue intervals from profiles/r06/valu_issue_rate.txt (tools/ubench/valu_rate.hip); fingerprint of the library's "
                      "sources %s = the loaded one" % (rel, library_fingerprint())}


def rocprof_launch_us(rel):
    """Average duration (us) of the full-resolution blur launches in the committed `rocprofv3 --kernel-trace --stats` summary of
    this command (tools/summarize_prof.py writes it beside the traffic), or None: when the file is missing, predates the
    field, or describes a library of other sources.  bench.py prints it beside the live hipEvent figure so that the line and
    profiles/ cannot drift apart unnoticed."""
    try:
        tj = json.load(open(os.path.join(ROOT, rel)))
        if tj.get("library_fingerprint") != library_fingerprint():
            return None
        v = tj.get("rocprof_avg_launch_us_full_resolution")
        return float(v) if v else None
    except Exception:
        return None


def replayed_traffic(rel):
    """(bytes per launch, where from) of a committed rocprofv3 PMC summary (tools/summarize_prof.py) -- replayed only while it was
    taken from a library of the same sources as the loaded one and covers all six full-resolution launches of every image."""
    tfile = os.path.join(ROOT, rel)
    if not os.path.exists(tfile):
        return None, None
    try:
        tj = json.load(open(tfile))
        if tj.get("library_fingerprint") != library_fingerprint():
            return None, ("%s was taken from a library with other sources (fingerprint %s, loaded %s): not replayed"
                          % (rel, tj.get("library_fingerprint"), library_fingerprint()))
        if tj.get("complete") and tj["launches_fetch_pass"] == 6 * tj["images_fetch_pass"] \
                and tj["launches_write_pass"] == 6 * tj["images_write_pass"]:
            return round(tj["traffic_bytes_per_launch"], 1), (
                "replayed from %s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, %d + %d launches = 6 per image, "
                "library fingerprint %s = the loaded one; not observed in this run)"
                % (rel, tj["launches_fetch_pass"], tj["launches_write_pass"], library_fingerprint()))
    except Exception:
        pass
    return None, None


def leg_c3(sp, torch, local_rank, size=16384, steps=3):
    """C3: one 16384^2 frame, all octaves, resident in HBM; its own blur and whole-call rooflines (N = 1 extras leg)."""
    plan = sp.SiftPlan(shape=(size, size), dtype=np.float32, device=local_rank, profile="light")
    t = torch.from_numpy(make_image(0, size)).cuda()
    for _ in range(5):       # (the frame took seconds to generate: ~25 ms of work bring the GPU's clocks back, tools/dev/ramp.py)
        kp = plan.keypoints(t)
    plan.profile_totals(reset=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    nk = 0
    for _ in range(steps):
        nk += len(plan.keypoints(t))
    torch.cuda.synchronize()
    el = (time.perf_counter() - t1) / steps
    tot = plan.profile_totals(reset=True)
    n_oct = int(plan.octave_max)
    blur_gbs = (8.0 * tot["blur0_pixels"] / 1e9) / (tot["blur0_ms"] / 1e3) if tot["blur0_ms"] > 0 else 0.0
    balg = bytes_alg(size, size, n_oct, nk / steps)
    del plan, t
    torch.cuda.empty_cache()
    c3_traffic, c3_src = replayed_traffic(PROFILE_DIR + "/blur_traffic_c3.json") if size == 16384 else (None, None)
    return {"ms_per_image": round(1e3 * el, 3), "value": round(size * size / 1e6 / el, 1), "unit": "Mpix/s", "steps": steps,
            "octaves": n_oct, "keypoints": int(nk / steps), "keypoints_per_s": round(nk / steps / el, 1),
            "roofline": {"bound": "hbm", "kernel": "blur_team_kernel: the 6 full-resolution launches per image (1 GiB planes)",
                         "achieved": round(blur_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(blur_gbs / HBM_PEAK_GBS, 4),
                         "avg_launch_us": round(1e3 * tot["blur0_ms"] / max(tot["blur0_launches"], 1), 1),
                         "alg_bytes_per_launch": 8.0 * size * size, "traffic": c3_traffic, "traffic_source": c3_src},
            "roofline_pipeline": {"bound": "hbm", "achieved": round(balg / el / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": round(balg / el / 1e9 / HBM_PEAK_GBS, 4), "bytes_alg_per_image": balg},
            "workload": "SiftPlan %dx%d fp32 uniform white noise, all %d octaves x 3 scales, input resident in HBM, records returned to host"
                        % (size, size, n_oct)}


def leg_c4(sp, torch, local_rank, steps=3, keep=None):
    """C4 on one GPU: the 64 x 2048^2 batch through a BatchPlan (16 lanes), records left in HBM as the exchange wants them.
    With `keep` (a list) the plans and frames are handed to the caller instead of being freed here: freeing 16 plans idles
    the GPU for longer than its clocks stay up."""
    frames = [torch.from_numpy(make_image(1000 + i, C4_SIZE)).cuda() for i in range(C4_FRAMES)]
    bp = sp.BatchPlan(shape=(C4_SIZE, C4_SIZE), dtype=np.float32, device=local_rank, profile="light")
    n_oct = int(bp.octave_max)
    for _ in range(2):
        counts, rec = bp.keypoints_batch_device(frames)
    torch.cuda.synchronize()
    times, blur = [], None
    for _ in range(steps):
        t1 = time.perf_counter()
        counts, rec = bp.keypoints_batch_device(frames)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t1)
        blur = bp.blur_times()
    el = sorted(times)[len(times) // 2]
    nk = int(sum(counts))
    balg = C4_FRAMES * bytes_alg(C4_SIZE, C4_SIZE, n_oct, nk / C4_FRAMES)
    blur_gbs = (8.0 * blur["blur0_pixels"] / 1e9) / (blur["blur0_ms"] / 1e3) if blur and blur["blur0_ms"] > 0 else 0.0
    lanes = bp.lanes
    if keep is not None:
        keep.append((bp, frames, rec))
    else:
        del bp, frames
        torch.cuda.empty_cache()
    return {"ms_per_batch": round(1e3 * el, 3), "ms_per_frame": round(1e3 * el / C4_FRAMES, 4),
            "value": round(C4_FRAMES * C4_SIZE * C4_SIZE / 1e6 / el, 1), "unit": "Mpix/s", "frames": C4_FRAMES, "lanes": lanes,
            "octaves": n_oct, "keypoints": nk, "keypoints_per_s": round(nk / el, 1),
            "roofline": {"bound": "hbm", "kernel": "the full-resolution (2048^2) blur launches of the batch; lanes overlap, so the "
                                                   "bracket of a launch group also holds other lanes' kernels",
                         "achieved": round(blur_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(blur_gbs / HBM_PEAK_GBS, 4),
                         "traffic": None},
            "roofline_pipeline": {"bound": "hbm", "achieved": round(balg / el / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": round(balg / el / 1e9 / HBM_PEAK_GBS, 4), "bytes_alg_per_batch": balg},
            "workload": "batch of %d frames of %dx%d fp32 white noise on ONE GPU (BASELINE configs[3] without the other 7 GPUs), "
                        "BatchPlan with %d lanes, frames resident in HBM, records left in HBM (keypoints_batch_device)"
                        % (C4_FRAMES, C4_SIZE, C4_SIZE, lanes)}


def leg_pipelined(sp, torch, size, n_oct, local_rank, keep=None):
    """The 2-lane BatchPlan leg; the LAST leg before the headline's warm-up at every N (the same kernels on the same frame
    size: the timed region starts from a GPU at its sustained clocks, N = 1 and N > 1 alike)."""
    out = {}
    # the pipelined path (BatchPlan): what a caller with a stack of frames gets from one GPU (last: the same
    #     kernels on the same frame size as the headline, whose warm-up follows directly)
    try:
        frames = [torch.from_numpy(make_image(i, size)).cuda() for i in range(8)] * 2
        bp = sp.BatchPlan(shape=(size, size), dtype=np.float32, device=local_rank, octave_max=n_oct, lanes=2)
        for _ in range(2):
            bp.keypoints_batch(frames)
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            t1 = time.perf_counter()
            res = bp.keypoints_batch(frames)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t1)
        tb = sorted(times)[len(times) // 2]
        out["pipelined"] = {"value": round(len(frames) * size * size / 1e6 / tb, 2), "unit": "Mpix/s",
                            "ms_per_frame": round(1e3 * tb / len(frames), 4), "frames_per_call": len(frames), "lanes": 2,
                            "keypoints": int(sum(len(r) for r in res)),
                            "note": "BatchPlan.keypoints_batch: frames pipelined over 2 plans; every frame bit-identical "
                                    "to SiftPlan.keypoints (tests/test_gpu_batch.py)"}
        if keep is not None:
            keep.append((bp, frames, res))      # freed by the caller after its timed region (freeing plans idles the GPU)
        del bp, frames
    except Exception as exc:
        out["pipelined"] = {"error": str(exc)[:200]}
    return out["pipelined"]


def extras(sp, torch, size, n_oct, local_rank):
    """Measurements beside the headline, N = 1 only, outside the timed region and never part of `value`."""
    out = {}
    # (2) host-to-host: the reference API takes host numpy arrays (plan.py:450-456); PCIe-inclusive, never `value`
    try:
        plan = sp.SiftPlan(shape=(size, size), dtype=np.float32, device=local_rank, octave_max=n_oct)
        host = make_image(3, size)
        pinned = torch.from_numpy(host).pin_memory().numpy()
        res = {}
        for name, img in (("pageable", host), ("pinned", pinned)):
            for _ in range(2):
                plan.keypoints(img)
            t1 = time.perf_counter()
            for _ in range(5):
                plan.keypoints(img)
            res[name] = (time.perf_counter() - t1) / 5
        out["host_to_host"] = {"ms_per_image_pageable_input": round(1e3 * res["pageable"], 4),
                               "ms_per_image_pinned_input": round(1e3 * res["pinned"], 4),
                               "value": round(size * size / 1e6 / res["pinned"], 2), "unit": "Mpix/s",
                               "note": "numpy image in, numpy recarray out: 64 MiB H->D over PCIe Gen5 x16 inside the call"}
        del plan
    except Exception as exc:
        out["host_to_host"] = {"error": str(exc)[:200]}
    # (2b) the keypoint-rich frame SURVEY 8(d) names as the input on which keypoints/s is meaningful: smoothed noise, seed 3,
    #      every octave -- about one keypoint per 108 pixels (the headline white noise: one per 1 500)
    try:
        from scipy.ndimage import gaussian_filter
        rich = gaussian_filter(np.random.default_rng(3).random((size, size)), 3.0).astype(np.float32)
        plan = sp.SiftPlan(shape=(size, size), dtype=np.float32, device=local_rank)
        t = torch.from_numpy(rich).cuda()
        for _ in range(3):
            kp = plan.keypoints(t)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(10):
            kp = plan.keypoints(t)
        el = (time.perf_counter() - t1) / 10
        out["keypoint_rich"] = {"ms_per_image": round(1e3 * el, 4), "keypoints": int(len(kp)), "keypoints_per_s": round(len(kp) / el, 1),
                                "value": round(size * size / 1e6 / el, 2), "unit": "Mpix/s", "octaves": int(plan.octave_max),
                                "input": "scipy.ndimage.gaussian_filter(default_rng(3).random((%d, %d)), 3.0) as float32, resident in HBM" % (size, size),
                                "note": "full gradient maps from the second call on (plan option maps = 2); records returned to the host"}
        del plan, t
    except Exception as exc:
        out["keypoint_rich"] = {"error": str(exc)[:200]}
    # (2c) the host-frame pipeline at the headline size: the reference API takes host numpy frames (plan.py:450-456); a
    #      BatchPlan uploads frame i+1 (pinned host memory, PCIe Gen5 x16) under the kernels of frame i
    try:
        nfr = 16
        hframes = [torch.from_numpy(make_image(40 + i, size)).pin_memory().numpy() for i in range(nfr)]
        best = None
        for lanes in (2, 3, 4):
            bp = sp.BatchPlan(shape=(size, size), dtype=np.float32, device=local_rank, octave_max=n_oct, lanes=lanes)
            bp.keypoints_batch(hframes)
            times = []
            for _ in range(3):
                t1 = time.perf_counter()
                res = bp.keypoints_batch(hframes)
                times.append(time.perf_counter() - t1)
            tb = sorted(times)[1]
            if best is None or tb < best[0]:
                best = (tb, lanes, int(sum(len(r) for r in res)))
            del bp
        tb, lanes, nk = best
        out["pipelined_host"] = {"ms_per_frame": round(1e3 * tb / nfr, 4), "value": round(nfr * size * size / 1e6 / tb, 2), "unit": "Mpix/s",
                                 "frames_per_call": nfr, "lanes": lanes, "keypoints": nk,
                                 "h2d_GBps": round(nfr * size * size * 4 / 1e9 / tb, 2),
                                 "note": "BatchPlan.keypoints_batch over %d pinned HOST frames (numpy in, numpy recarrays out): the 64 MiB "
                                         "upload of frame i+1 runs under the kernels of frame i; best of lanes = 2, 3, 4" % nfr}
        del hframes
    except Exception as exc:
        out["pipelined_host"] = {"error": str(exc)[:200]}
    # (3) MatchPlan, BASELINE.json configs[4]: 100k x 100k 128-D uint8 descriptors, L1 + ratio test as the reference
    try:
        n = 100000
        rng = np.random.default_rng(1)
        a = np.zeros(n, sp.MatchPlan.dtype_kp); a["desc"] = rng.integers(0, 256, (n, 128), dtype=np.uint8)
        b = np.zeros(n, sp.MatchPlan.dtype_kp)
        perm = rng.permutation(n); half = n // 2
        b["desc"][:half] = np.clip(a["desc"][perm[:half]].astype(np.int16) + rng.integers(-8, 9, (half, 128)), 0, 255).astype(np.uint8)
        b["desc"][half:] = rng.integers(0, 256, (n - half, 128), dtype=np.uint8)
        mp = sp.MatchPlan(size=n, device=local_rank)
        ta = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda(); tb_ = torch.from_numpy(b.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()
        mp.match(ta, tb_, raw_results=True)
        t1 = time.perf_counter()
        pairs = mp.match(ta, tb_, raw_results=True)
        el = time.perf_counter() - t1
        ms = mp.kernel_ms()
        out["match_100k"] = {"kernel_ms": round(ms, 3), "call_ms_device_lists": round(1e3 * el, 3), "pairs": int(len(pairs)),
                             "expected_pairs": half, "descriptor_pairs_per_s": round(float(n) * n / (ms / 1e3), 1),
                             "byte_sad_per_s": round(float(n) * n * 128 / (ms / 1e3), 1),
                             "note": "brute-force L1 + 0.73^2 ratio test, both lists resident in HBM"}
    except Exception as exc:
        out["match_100k"] = {"error": str(exc)[:200]}
    # (2d) BASELINE.json configs[2]: SiftPlan 16384 x 16384 fp32, every octave -- the configuration whose planes (1 GiB each)
    #      do not fit the 256 MiB Infinity Cache, i.e. where the HBM roofline is about HBM
    try:
        out["c3_16384"] = leg_c3(sp, torch, local_rank)
    except Exception as exc:
        out["c3_16384"] = {"error": str(exc)[:200]}
    # (2e) BASELINE.json configs[3] on this one GPU: 64 frames of 2048 x 2048 through a BatchPlan
    try:
        out["c4_one_gpu"] = leg_c4(sp, torch, local_rank)
    except Exception as exc:
        out["c4_one_gpu"] = {"error": str(exc)[:200]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c2", choices=["c2", "c4"],
                    help="c2: one 4096^2 frame per step and GPU (default, the headline); c4: 64 x 2048^2 frames sharded over the GPUs")
    ap.add_argument("--size", type=int, default=0, help="image side (default: the BASELINE config: 4096 for c2, 2048 for c4)")
    ap.add_argument("--octaves", type=int, default=-1, help="0 = every octave (reference default); default 3 for c2, all for c4")
    ap.add_argument("--full", action="store_true",
                    help="also the measurements beside the headline: the legs (BatchPlan, host-to-host, MatchPlan, C3, C4), "
                         "`steady` and the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write what the last timed step returned to DIR/<name>.npy (float32 / float64, at most 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-steady", action="store_true", help="with --full: skip the 200-step steady-state measurement after the timed region")
    ap.add_argument("--no-pipelined", "--no-extras", dest="no_extras", action="store_true",
                    help="skip the extra measurements (BatchPlan, host-to-host, MatchPlan) with --full, the clock ramp without it")
    ap.add_argument("--backend", default="", help="torch.distributed backend (default nccl = RCCL; gloo only with --share-gpu)")
    ap.add_argument("--share-gpu", action="store_true", help="rehearsal only: every rank uses cuda:0")
    args = ap.parse_args()
    if args.dump_outputs and args.steps < 1:
        ap.error("--dump-outputs needs at least one timed step")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device is visible (there is no CPU fallback)")
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    distributed = world > 1
    # RCCL refuses two ranks on one device, so the one-GPU rehearsal of the N>1 path runs its collectives over gloo
    backend = args.backend or ("gloo" if args.share_gpu else "nccl")
    xdev = torch.device("cuda", local_rank) if backend == "nccl" else torch.device("cpu")
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=backend)
        world_observed = dist.get_world_size()
    else:
        world_observed = 1

    import ctypes
    import sift_pyocl_amd as sp
    from sift_pyocl_amd import _lib
    from sift_pyocl_amd.batch import RECORD_BYTES, gather_records_device, shard_indices, split_gathered

    c4 = args.config == "c4"
    size = args.size or (C4_SIZE if c4 else SIZE)
    octaves = args.octaves if args.octaves >= 0 else (0 if c4 else OCTAVES)
    K, W = args.steps, args.warmup

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    def xfer(t):           # device tensor -> the collective's device (identity for nccl)
        return t if t.device == xdev else t.to(xdev)

    result = {}
    extra = {}
    keepalive = []          # what the last leg before the timed region allocated: freed after the region, not before it
    order = "W warm-up + K timed steps first"
    if c4:
        # ---------------------------------------------------------------- C4: 64 x 2048^2 sharded over the ranks
        mine = shard_indices(C4_FRAMES, rank, world)
        frames = [torch.from_numpy(make_image(1000 + i, size)).cuda() for i in mine]
        bp = sp.BatchPlan(shape=(size, size), dtype=np.float32, device=local_rank, octave_max=octaves or None, profile="light")
        n_oct = bp.octave_max
        torch.cuda.synchronize()

        def step():
            counts, records = bp.keypoints_batch_device(frames)
            if distributed:
                all_counts, gathered = gather_records_device(counts, xfer(records), C4_FRAMES, rank, world)
                return sum(sum(r) for r in all_counts), (all_counts, gathered)
            return sum(counts), (counts, records)

        for _ in range(max(W, 1)):
            step()
        barrier()
        t0 = time.perf_counter()
        total_kp = 0
        for _ in range(K):
            nk, keep = step()
            total_kp += nk
        barrier()
        elapsed = time.perf_counter() - t0
        if args.dump_outputs and rank == 0:
            if distributed:
                outputs = split_gathered(keep[0], keep[1], C4_FRAMES, world)
            else:
                host = keep[1].cpu().numpy()
                bounds = np.cumsum([0] + list(keep[0])) * RECORD_BYTES
                outputs = [host[a:b].view(sp.SiftPlan.dtype_kp) for a, b in zip(bounds[:-1], bounds[1:])]
        units = K * C4_FRAMES * size * size / 1e6
        workload = ("batch of %d frames of %dx%d fp32 uniform white noise, frame i on rank i mod %d (%d per GPU), BatchPlan "
                    "(%d lanes) per rank, frames resident in HBM, all-gather of every frame's records on device tensors"
                    % (C4_FRAMES, size, size, world, len(mine), bp.lanes))
        result.update(scaling="strong", images_per_step=C4_FRAMES, kp_per_img=total_kp / max(K, 1) / C4_FRAMES, n_oct=n_oct)
        kt = None
        try:
            c4_blur = bp.blur_times()          # rank 0's lanes, last batch: brackets around each frame's full-resolution blur launches
        except Exception:
            c4_blur = None
    else:
        # ---------------------------------------------------------------- C2: one 4096^2 frame per step and GPU
        plan = sp.SiftPlan(shape=(size, size), dtype=np.float32, devicetype="GPU", device=local_rank, profile="light",
                           octave_max=octaves or None)
        n_oct = plan.octave_max
        # distinct frames in rotation: every one of them is seen by the warm-up steps (the first call on a new device
        # buffer costs ~80 us more than the following ones, whatever the cause -- it is not part of a steady-state step)
        n_img = max(1, min(K, 8, W if W > 0 else 1))
        dev_images = [torch.from_numpy(make_image(rank * 1000 + i, size)).cuda() for i in range(n_img)]
        torch.cuda.synchronize()

        # N > 1 (SURVEY 8d "C2-scaling": total Mpix / wall time INCLUDING the final all-gather of every image's records):
        # each step's records are kept where the descriptor kernels left them -- one device-to-device copy out of the plan's
        # list into this rank's arena -- and ONE exchange at the end of the timed region gathers the records of all K frames
        # of all ranks on device tensors (counts, then the padded record bytes): no host staging.
        kept = {"counts": [], "used": 0, "arena": None}

        def keep_records():
            rec_view = plan.device_records()
            n = rec_view.count
            need = kept["used"] + n * 144
            if kept["arena"] is None or need > kept["arena"].numel():
                grown = torch.empty(max(need * 2, (K + 1) * max(n, 1024) * 216), dtype=torch.uint8, device=torch.device("cuda", local_rank))
                if kept["used"]:
                    grown[:kept["used"]] = kept["arena"][:kept["used"]]
                kept["arena"] = grown
            if n:
                # one D->D copy out of the plan's list, by the library itself (siftmi_plan_fetch with a device destination:
                # 13 us per step; a torch slice assignment of the same bytes: 22 us -- tools/dev/keep_cost.py)
                _lib.check(_lib.lib().siftmi_plan_fetch(plan._handle, ctypes.c_void_p(kept["arena"].data_ptr() + kept["used"]), 1, 0, n))
            kept["counts"].append(n)
            kept["used"] = need

        def exchange():
            counts, used = kept["counts"], kept["used"]
            out = gather_records_device(counts, xfer(kept["arena"][:used]), len(counts) * world, rank, world)
            kept["counts"], kept["used"] = [], 0
            return out, used

        # The legs beside the headline run FIRST (N = 1): they are not part of any timed step either way, and the W warm-up
        # + K timed steps that follow then start from a GPU at its sustained clocks instead of from seconds of idle time
        # (tools/dev/ramp.py: after 0.2 ... 2 s of idle the first ~25 calls run 0.92, 0.85, 0.83, 0.81, 0.80 ms in groups of
        # five before the 0.79 of the steady state; rounds 1-4 ran the legs after the timed region and their lines carry that
        # ramp: compare `steady` across rounds, not `ms_per_step`).  Nothing of the timed region changes.  A plain run has no
        # legs: the headline call itself, repeated for RAMP_S seconds, brings the clocks up instead.
        last = None
        if args.full and not args.no_extras:
            if world == 1:
                extra = extras(sp, torch, size, n_oct, local_rank)
            # every rank, at every N: the 2-lane BatchPlan leg directly in front of the warm-up (reported by rank 0)
            extra["pipelined"] = leg_pipelined(sp, torch, size, n_oct, local_rank, keep=keepalive)
            order = ("legs beside the headline first (N > 1: the pipelined leg only, on every rank), then W warm-up + K timed "
                     "steps, then `steady` (N = 1), then the CPU baselines (N = 1)")
        elif not args.no_extras:
            t_end, i = time.perf_counter() + RAMP_S, 0
            while time.perf_counter() < t_end:
                last = plan.keypoints(dev_images[i % n_img])
                i += 1
            order = "%d untimed calls (%.1f s: the clock ramp), then W warm-up + K timed steps" % (i, RAMP_S)
        else:
            order = "W warm-up + K timed steps first"
        for i in range(W):
            # held like in the timed loop: the previous result is alive while the next call runs, so the pinned pool serves
            # two record blocks in rotation (without this the second TIMED step allocated the second block: +0.3 ms once)
            last = plan.keypoints(dev_images[i % n_img])
            if distributed:
                keep_records()
        if distributed:
            exchange()
        blur_ms = blur_px = tot_ms = b0_ms = b0_px = 0.0
        b0_launches = 0
        n_kp = 0
        plan.profile_totals(reset=True)
        barrier()
        t0 = time.perf_counter()
        exchange_ms = exchange_bytes = None
        marks = []
        for i in range(K):
            last = plan.keypoints(dev_images[i % n_img])
            n_kp += len(last)
            if distributed:
                keep_records()
            marks.append(time.perf_counter())
        if distributed:
            torch.cuda.synchronize()
            te = time.perf_counter()
            (all_counts, gathered), exchange_bytes = exchange()
            torch.cuda.synchronize()
            exchange_ms = (time.perf_counter() - te) * 1e3
            assert sum(sum(r) for r in all_counts) >= n_kp and gathered.shape[0] == world
        barrier()
        elapsed = time.perf_counter() - t0
        outputs = [np.array(last)] if args.dump_outputs else None    # a copy: the next call may reuse the pinned record block
        # hipEvent times of the K timed calls (the library sums them as the calls complete: one read-out, after the region)
        t = plan.profile_totals(reset=True)
        assert t["calls"] == K
        if os.environ.get("BENCH_STEP_TIMES"):
            print("step ms:", " ".join("%.3f" % (1e3 * (b - a)) for a, b in zip([t0] + marks[:-1], marks)), file=sys.stderr)
        tot_ms = t["total_ms"]; b0_ms = t["blur0_ms"]; b0_px = t["blur0_pixels"]; b0_launches = t["blur0_launches"]
        total_kp = n_kp
        # beside `value`: the same step over a longer window -- reported, never `value` (rounds 1-4, whose timed region
        # started from an idle GPU, printed 3-5 % more in `ms_per_step` than here: this is the figure to compare across rounds)
        steady = None
        if world == 1 and args.full and not args.no_steady:
            ns = 200
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i in range(ns):
                plan.keypoints(dev_images[i % n_img])
            torch.cuda.synchronize()
            steady = {"ms_per_step_steady": round(1e3 * (time.perf_counter() - t1) / ns, 4), "steps": ns,
                      "note": "same call, %d further steps right after the timed region" % ns}
        keepalive.clear()
        units = world * K * size * size / 1e6
        workload = ("SiftPlan %dx%d fp32 uniform white noise (numpy default_rng(seed).random), %d octaves x 3 scales, input "
                    "resident in HBM, records returned to host" % (size, size, n_oct))
        result.update(scaling="weak", images_per_step=world, kp_per_img=n_kp / max(K, 1), n_oct=n_oct,
                      exchange_ms=None if exchange_ms is None else round(exchange_ms, 3), exchange_bytes=exchange_bytes)
        kt = dict(b0_ms=b0_ms, b0_px=b0_px, b0_launches=b0_launches, tot_ms=tot_ms, steady=steady)

    rank_ms = None
    if distributed:
        # every rank's own time of the region (the reported one is their maximum): a first multi-GPU curve can then be read
        # without a re-run -- a slow rank, a slow link and a uniform slow-down look different here
        mine_el = torch.tensor([elapsed], dtype=torch.float64, device=xdev)
        all_el = [torch.zeros_like(mine_el) for _ in range(world)]
        dist.all_gather(all_el, mine_el)
        rank_ms = [1e3 * float(t.item()) / max(K, 1) for t in all_el]
        el = torch.tensor([elapsed], dtype=torch.float64, device=xdev)
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        elapsed = float(el.item())
        if not c4:
            tk = torch.tensor([float(total_kp)], dtype=torch.float64, device=xdev)
            dist.all_reduce(tk, op=dist.ReduceOp.SUM)
            total_kp = float(tk.item())

    if rank == 0:
        out = {
            "metric": "SiftPlan.keypoints throughput, %dx%d fp32 (Mpix/s; keypoints/s in keypoints_per_s)" % (size, size),
            "value": round(units / elapsed, 2), "unit": "Mpix/s",
            "keypoints_per_s": round(total_kp / elapsed, 1),
            "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": round(1e3 * elapsed / max(K, 1), 4),
            "higher_is_better": True, "scaling": result["scaling"], "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": workload, "name": args.config, "octaves": result["n_oct"], "scales": 3,
                       "keypoints_per_image": round(result["kp_per_img"], 1), "images_per_step": result["images_per_step"],
                       "exchange": ("all_gather of keypoint records on device tensors, backend %s, world size %d as seen by "
                                    "torch.distributed" % (backend, world_observed)) if distributed else "none",
                       "exchange_ms": result.get("exchange_ms"), "exchange_bytes_per_rank": result.get("exchange_bytes"),
                       "backend": backend if distributed else None, "world_size_observed": world_observed},
        }
        if rank_ms is not None:
            out["ms_per_step_ranks"] = {"min": round(min(rank_ms), 4), "max": round(max(rank_ms), 4), "per_rank": [round(v, 4) for v in rank_ms],
                                        "note": "each rank's own wall time of the timed region / K; `ms_per_step` is the maximum"}
        if kt is not None:
            blur_gbs = (8.0 * kt["b0_px"] / 1e9) / (kt["b0_ms"] / 1e3) if kt["b0_ms"] > 0 else 0.0
            # HBM traffic per full-resolution blur launch: not observable from inside this process -- replayed from the
            # committed rocprofv3 PMC passes of this same command (FETCH_SIZE x2 + WRITE_SIZE, tools/summarize_prof.py)
            # -- and only while the summary was taken from a library of the same sources as the loaded one (its fingerprint)
            traffic, traffic_src = (None, None)
            if size == SIZE and result["n_oct"] == OCTAVES:
                traffic, traffic_src = replayed_traffic(PROFILE_DIR + "/blur_traffic.json")
            # whole call: algorithmic bytes of an image over the wall time of a step (the light profile brackets only the blur
            # launches: every further event record between kernels would be a bubble in the timed region)
            pipe_ms = kt["tot_ms"] if kt["tot_ms"] > 0 else 1e3 * elapsed
            pipe_gbs = (bytes_alg(size, size, result["n_oct"], result["kp_per_img"]) * K / 1e9) / (pipe_ms / 1e3) if pipe_ms > 0 else 0.0
            rp_us = rocprof_launch_us(PROFILE_DIR + "/blur_traffic.json") if (size == SIZE and result["n_oct"] == OCTAVES) else None
            rp_gbs = (8.0 * size * size / 1e9) / (rp_us / 1e6) if rp_us else None
            out["roofline"] = {
                "bound": "hbm",
                "kernel": "blur_team_kernel<N, NORM, S> (fused separable Gaussian blur): the %d full-resolution (octave 0) "
                          "launches per image, initial blur + 5 scales (79 %% of all blur bytes at 3 octaves); they never "
                          "overlap another kernel, later octaves run concurrently with the detection streams"
                          % (kt["b0_launches"] // max(K, 1)),
                "achieved": round(blur_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(blur_gbs / HBM_PEAK_GBS, 4),
                # SURVEY 8(d)'s own definition, with equal standing: algorithmic bytes of a whole call over the time of its kernels
                "frac_pipeline": round(pipe_gbs / HBM_PEAK_GBS, 4), "achieved_pipeline": round(pipe_gbs, 1),
                # the dominant kernel's fraction again, from the COMMITTED rocprofv3 kernel stats of this command (null when
                # that summary describes other sources than the loaded library's)
                "frac_rocprof": None if rp_gbs is None else round(rp_gbs / HBM_PEAK_GBS, 4),
                "avg_launch_us_rocprof": None if rp_us is None else round(rp_us, 2),
                "traffic": traffic, "traffic_source": traffic_src,
                "avg_launch_us": round(1e3 * kt["b0_ms"] / max(kt["b0_launches"], 1), 2),
                "alg_bytes_per_launch": round(8.0 * kt["b0_px"] / max(kt["b0_launches"], 1), 1),
                "timing": "frac / achieved: one hipEvent pair on the plan's pyramid stream around the 6 back-to-back launches "
                          "(inter-kernel gaps included), live; frac_pipeline: bytes_alg of an image (roofline_pipeline) over the "
                          "hipEvent time first -> last kernel of a call, live; frac_rocprof: 8 B/px over the average duration of "
                          "the same launches in %s/rocprofv3_summary.txt (a traced run of --steps 10 --warmup 2: shorter, on the "
                          "clock ramp, hence below the live figure)" % PROFILE_DIR}
            out["roofline_pipeline"] = {"bound": "hbm", "achieved": round(pipe_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                        "frac": round(pipe_gbs / HBM_PEAK_GBS, 4),
                                        "ms_per_image": round(pipe_ms / max(K, 1), 4), "time": "hipEvent first -> last kernel" if kt["tot_ms"] > 0 else "wall clock of the timed steps",
                                        "bytes_alg_per_image": bytes_alg(size, size, result["n_oct"], result["kp_per_img"])}
        if c4:
            # the batch's rooflines, at every N: the dominant kernel from rank 0's own light-profile brackets (its lanes overlap, so
            # a bracket also holds other lanes' kernels: a lower bound of the kernel's rate), the whole job from the wall clock
            balg = C4_FRAMES * bytes_alg(size, size, result["n_oct"], result["kp_per_img"])
            pipe_gbs = balg * K / 1e9 / elapsed if elapsed > 0 else 0.0
            blur_gbs = (8.0 * c4_blur["blur0_pixels"] / 1e9) / (c4_blur["blur0_ms"] / 1e3) if c4_blur and c4_blur.get("blur0_ms", 0) > 0 else 0.0
            out["roofline"] = {"bound": "hbm", "kernel": "the full-resolution (%dx%d) blur launches of rank 0's share of the batch (light-profile "
                                                         "brackets of its lanes, last step; lanes overlap)" % (size, size),
                               "achieved": round(blur_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(blur_gbs / HBM_PEAK_GBS, 4),
                               "frac_pipeline": round(pipe_gbs / HBM_PEAK_GBS / max(world, 1), 4), "achieved_pipeline": round(pipe_gbs, 1),
                               "traffic": None,
                               "timing": "frac_pipeline: algorithmic bytes of the whole batch over the wall time of a step, per GPU (divided by N)"}
        if kt is not None and size == SIZE and result["n_oct"] == OCTAVES and world == 1:
            rv = roofline_valu(1e3 * elapsed / max(K, 1))
            if rv is not None:
                out["roofline_valu"] = rv
        if kt is not None and kt.get("steady"):
            out["steady"] = kt["steady"]
        out["order"] = order
        out.update(extra)
        if args.dump_outputs:
            rows = dump_outputs(args.dump_outputs, outputs)
            print("bench.py: %d keypoint rows of the last timed step written to %s" % (rows, args.dump_outputs), file=sys.stderr)
        if args.full and not args.no_cpu_baseline and world == 1 and not c4:
            out["cpu_baseline"] = cpu_baseline(size, result["n_oct"])
            ref = cpu_reference_kernels(size, result["n_oct"])
            if ref is not None:
                out["cpu_baseline_reference_kernels"] = ref
        print(json.dumps(out), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
