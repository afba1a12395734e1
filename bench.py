#!/usr/bin/env python3
"""bench.py -- frames/sec of the Betapose per-frame inference hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W          (N>1: launched by torch.distributed.run)

One "step" = one pass of the hot path over one batch (default batch 1 = BASELINE.json
configs[1]) of synthetic 640x480 BGR u8 frames that are already resident in HBM:
  device (one hipGraph): Pillow-exact bicubic stretch to 416^2 -> YOLOv3 (fp32-accurate bf16x3 MFMA) ->
      decode + arg-max objectness -> box rescale + crop 320x256 -> FastPose (SE-ResNet-101 + DUC)
      -> heat-map arg-max -> 316-float record
  host: D2H of the record, key-point decoding, pPose-NMS, PnP  (software-pipelined one step deep)
Weights are seeded random tensors of the reference architectures (no checkpoints ship).
Frames shard by image: each rank runs its own frames (weak scaling), weights are broadcast from
rank 0 over RCCL at start-up and the per-frame result records are all-gathered at the end.

Prints ONE JSON line (rank 0).  A plain run sets up, runs the W warm-up steps, times the K steps and reports them
("latency_ms" = per-frame p50 / p95 with all frames in flight, "rccl" for N > 1).  With --full the line also carries:
"repeats" / "value_settled" (more K-step regions back to back), "roofline" (conv FLOPs of the timed region over its wall
clock = the in-situ figure, plus the dominant kernel alone with HIP events), one-frame-at-a-time latency, clocks under load,
"h2d_inclusive" (the same run with every frame uploaded from pinned host memory inside the timed region -- never `value`),
the other precisions and served configurations, the flip rate and "cpu_baseline" (oracle on the host cores); all N = 1 only
except "repeats" and "roofline".

--dump-outputs DIR writes what the timed path returned for the LAST timed step (rank 0's frames) as DIR/<name>.npy.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_F16_MFMA_TFLOPS = 2500.0   # MI355X_MICROARCH.md: BF16/F16 ~2.5 PF dense (v_mfma_f32_32x32x16_f16)
PEAK_BF16X3_TFLOPS = 2500.0 / 6  # fp32-accurate mode: six bf16 MFMA products per algorithmic multiply
PEAK_HBM_GBPS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s peak (~6.3 TB/s achievable)
TILE_NAMES = {0: "1, 1", 1: "2, 1", 2: "1, 1", 3: "1, 2", 5: "2, 1", 6: "2, 2"}
# conv_pl.hip instantiations (csrc/conv_pl.hip launch_pl_np): tile id -> {planes: "WM, WN, TM, TN, NST, CPS"}
PL_TILE_ARGS = {13: {3: "2, 2, 1, 1, 3, 1", 1: "2, 2, 1, 1, 3, 2"}, 14: {3: "2, 2, 2, 2, 3, 1", 1: "2, 2, 2, 2, 4, 1"},
                15: {3: "2, 2, 2, 1, 3, 1", 1: "2, 2, 2, 1, 3, 2"}, 16: {3: "4, 2, 2, 2, 2, 1", 1: "4, 2, 2, 2, 3, 2"}}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1, help="frames per step (1 = the reference's own batch)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--prefetch", action="store_true", help="lone-frame latency mode for the main run too (bp_*_set_prefetch): pays with --streams 1 only")
    ap.add_argument("--fixed-box", action="store_true", help="deterministic crop box (220,140,420,340)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--other-modes", default="f32,f16",
                    help="N=1 only: after the timed region, also time a short run of these matrix-core operand modes on "
                         "the same workload and report them under \"other_precisions\" (never as \"value\"); '' = skip")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-side-runs", action="store_true", help="skip the one-frame-at-a-time and H2D-inclusive runs")
    ap.add_argument("--no-flip-rate", action="store_true", help="skip the planted-margin flip-rate object")
    ap.add_argument("--no-served-legs", action="store_true", help="skip the configs[2] leg (fp16, 28 frames per launch x 3 streams) and the other_configs lines")
    ap.add_argument("--repeats", type=int, default=None,
                    help="--full: K-step timed regions run back to back (default 5): `value` is the FIRST (the contract's region), "
                         "\"repeats\" reports p50 / min / max over all of them")
    ap.add_argument("--insitu", default="", metavar="PATH",
                    help="--full, N=1: after the timed regions, time every convolution WHILE the frames are in flight (s_memtime "
                         "stamps written by the kernels themselves) and write the per-layer table to PATH")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, run every other measurement of the line (repeats, side runs, roofline, other "
                         "precisions, served legs, flip rate, CPU baseline; each still switched off by its --no-* option)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the arrays the timed path returned in its last timed step as DIR/<name>.npy")
    ap.add_argument("--partition", type=int, default=0,
                    help="give each of the --streams frames in flight its own 1/PARTITION slice of the CUs of every "
                         "XCD (hipExtStreamCreateWithCUMask); 0 = ordinary streams sharing the chip")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--pool", type=int, default=8, help="distinct synthetic frames per rank")
    ap.add_argument("--streams", type=int, default=4,
                    help="frames in flight per GPU: independent batch-1 passes on separate HIP streams (engine clones "
                         "share the filters); 1 = strictly one frame at a time")
    ap.add_argument("--sk-target", type=int, default=512)
    ap.add_argument("--sk-min", type=int, default=4)
    ap.add_argument("--sk-max", type=int, default=8)
    ap.add_argument("--tile", type=int, default=-1)
    ap.add_argument("--precision", choices=["f32", "f16", "f16r", "bf16x3"], default="bf16x3",
                    help="matrix-core operand precision: bf16x3 = fp32-accurate 3-way bf16 operand split (default, parity-grade); f32 = fp32 MFMA; f16 = fp16 "
                         "MFMA operands with fp32 accumulation (BASELINE configs[2])")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be >= 1")
    if not a.full and ((a.repeats or 1) > 1 or a.insitu):
        ap.error("--repeats > 1 and --insitu are measurements beyond the headline: add --full")
    if a.repeats is None:
        a.repeats = 5 if a.full else 1
    return a


def cpu_baseline(seconds: float, kp3d, cam_K):
    """The oracle (torch-CPU / numpy restatement of the reference path) timed on this box's host cores."""
    import torch
    from PIL import Image
    from betapose_amd import cfg as C, synth, weights as W
    from oracle import kpd_ref, post_ref, yolo_ref
    # torch-CPU conv scales to ~16 threads on this path and collapses beyond (256 threads: >100 s/frame on the
    # EPYC 9575F box), so the baseline runs on min(16, cores) threads; that count is what "cores" reports
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    blocks = C.parse_cfg_text(C.yolov3_single_cfg_text())
    convs = W.split_darknet_stream(blocks, synth.synth_yolo_stream(1, blocks))
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_fastpose_state_dict(2).items()}
    for c in convs:   # tensors once, not per frame
        for k in list(c.keys()):
            if isinstance(c[k], np.ndarray):
                c[k] = np.ascontiguousarray(c[k])
    im_dim = torch.tensor([[640.0, 480.0, 640.0, 480.0]])

    def one(frame):
        img = Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).resize((416, 416), 3)
        x = torch.from_numpy(np.asarray(img, dtype=np.uint8).transpose(2, 0, 1).copy()).float().div(255).unsqueeze(0)
        pred = yolo_ref.darknet_forward(blocks, convs, x)
        dets = yolo_ref.write_results(pred, 0.01, 80)
        if isinstance(dets, int):
            return None
        boxes, scores = yolo_ref.rescale_boxes(dets, im_dim, 416)
        inps, pt1, pt2 = post_ref.crop_from_dets_frame(frame, boxes)
        hm = kpd_ref.fastpose_forward(sd, inps)
        _, preds_img, preds_scores = post_ref.get_prediction(hm, pt1, pt2)
        res = post_ref.pose_nms(boxes, scores, preds_img, preds_scores)
        if res:
            post_ref.solve_pnp_iterative_ref(kp3d, res[0]["keypoints"].numpy(), cam_K)
        return res

    frames = synth.synth_frames(16, 1234)
    one(frames[0])   # warm-up
    n, t0 = 0, time.perf_counter()
    while True:
        one(frames[n % len(frames)])
        n += 1
        el = time.perf_counter() - t0
        if el >= seconds or n >= 400:
            break
    ref = reference_darknet_c(frames, blocks, torch.get_num_threads())
    return {"value": n / el, "unit": "frames/sec", "cores": torch.get_num_threads(), "host_cores": os.cpu_count(), "kind": "port",
            "cores_note": "`cores` = threads the oracle ran on (torch-CPU convolutions scale to ~16 threads on this path and collapse beyond); "
                          "`host_cores` = logical CPUs of the box",
            "reference_darknet_c": ref,
            "sample": "%d synthetic 640x480 frames through oracle/ (PIL resize, torch-CPU fp32 YOLOv3+FastPose, "
                      "getPrediction, pose_nms, SOLVEPNP_ITERATIVE restatement) in %.1f s" % (n, el),
            "cpu_model": _cpu_model()}


class _quiet_c_output:
    """Darknet-C prints its layer table with printf/fprintf: keep stdout to the one JSON line."""

    def __enter__(self):
        sys.stdout.flush(); sys.stderr.flush()
        self._saved = (os.dup(1), os.dup(2))
        null = os.open(os.devnull, os.O_WRONLY)
        os.dup2(null, 1); os.dup2(null, 2)
        os.close(null)

    def __exit__(self, *exc):
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        os.dup2(self._saved[0], 1); os.dup2(self._saved[1], 2)
        os.close(self._saved[0]); os.close(self._saved[1])
        return False


def reference_darknet_c(frames, blocks, threads):
    """The reference's OWN detector executable code (Darknet-C compiled into oracle/_ref by oracle/Makefile) timed on
    the same host cores: YOLO forward + get_network_boxes only -- the KPD half of the reference is Python and cannot
    travel to this box.  None when oracle/_ref was not built."""
    import ctypes
    import tempfile
    from PIL import Image
    from betapose_amd import cfg as C, synth, weights as W
    from oracle import darknet_c_ref
    if not darknet_c_ref.available():
        return None
    try:
        ctypes.CDLL("libgomp.so.1").omp_set_num_threads(int(threads))
    except OSError:
        pass
    with tempfile.TemporaryDirectory(prefix="bp_dk_") as tmp, _quiet_c_output():
        wpath = os.path.join(tmp, "01.weights")
        W.write_darknet_weights(wpath, synth.synth_yolo_stream(1, blocks))
        net = darknet_c_ref.DarknetC(C.yolov3_single_cfg_text(), wpath, 416)
        xs = [np.asarray(Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).resize((416, 416), 3),
                         dtype=np.float32).transpose(2, 0, 1) / 255.0 for f in frames[:16]]
        net.predict_rows(np.ascontiguousarray(xs[0]))   # warm-up
        t0 = time.perf_counter()
        for x in xs:
            net.predict_rows(np.ascontiguousarray(x))
        el = time.perf_counter() - t0
    return {"yolo_frames_per_sec": len(xs) / el, "threads": int(threads), "kind": "reference",
            "sample": "%d frames, network_predict_image + get_network_boxes of the reference's Darknet-C (AVX2, OpenMP)" % len(xs)}


class ClockSampler:
    """Shader clock and package power WHILE the timed regions run (a thread polling `rocm-smi --showclocks --showpower`):
    with several frames in flight this pipeline runs into the package power limit and the shader clock drops below its
    2.4 GHz ceiling -- frames/s then follow the clock, not the kernels' latency."""

    def __init__(self, period=0.5):
        import threading
        self.period, self.samples, self._stop = period, [], threading.Event()
        self._t = threading.Thread(target=self._loop, daemon=True)
        self.before = self.after = None
        self.t_before = self.t_after = 0.0

    @staticmethod
    def _smi_json(*flags):
        import subprocess
        try:
            out = subprocess.run(["amd-smi", "metric", "-g", "0", *flags, "--json"], capture_output=True, text=True, timeout=10).stdout
            d = json.loads(out[out.index("{"):])
            d = d.get("gpu_data", d) if isinstance(d, dict) else d
            return d[0] if isinstance(d, list) else d
        except Exception:
            return None

    @classmethod
    def _snapshot(cls):
        """The SMU's throttle accumulators (one count per sample interval in which the limiter was active) and the socket's
        energy counter: amd-smi metric --throttle / --energy."""
        snap = {}
        t = cls._smi_json("--throttle")
        if t and isinstance(t.get("throttle"), dict):
            for k, v in t["throttle"].items():
                if k.endswith("_accumulated") or k == "accumulation_counter":
                    if isinstance(v, dict):            # per XCC: {"xcp_0": [...]}
                        v = [x for lst in v.values() if isinstance(lst, list) for x in lst if isinstance(x, (int, float))]
                        v = sum(v) / len(v) if v else None
                    if isinstance(v, (int, float)):
                        snap[k] = float(v)
        e = cls._smi_json("--energy")
        try:
            snap["energy_J"] = float(e["energy"]["total_energy_consumption"]["value"])
        except Exception:
            pass
        return snap

    def _loop(self):
        import re
        import subprocess
        while not self._stop.is_set():
            try:
                out = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=5).stdout
                m1 = re.search(r"GPU\[0\]\s*:\s*sclk clock level[^(]*\((\d+)Mhz\)", out)
                m2 = re.search(r"GPU\[0\]\s*:[^\n]*Power \(W\):\s*([0-9.]+)", out)
                if m1 and m2:
                    self.samples.append((int(m1.group(1)), float(m2.group(1))))
            except Exception:
                pass
            self._stop.wait(self.period)

    def __enter__(self):
        self.before, self.t_before = self._snapshot(), time.perf_counter()
        self._t.start()
        return self

    def __exit__(self, *exc):
        self.after, self.t_after = self._snapshot(), time.perf_counter()
        self._stop.set()
        self._t.join(timeout=6)

    def limits(self, frames):
        """Which limiter the SMU reports for the sampled window (accumulator deltas over the window's sample count) and the
        socket energy per frame.  None when amd-smi gave nothing."""
        if not self.before or not self.after:
            return None
        n = self.after.get("accumulation_counter", 0.0) - self.before.get("accumulation_counter", 0.0)
        out = {"window_s": round(self.t_after - self.t_before, 2), "smu_samples": int(n)}
        active = {}
        for k, v in self.after.items():
            if k.endswith("_accumulated") and k in self.before:
                d = v - self.before[k]
                if d > 0:
                    active[k[:-len("_accumulated")]] = round(d / n, 4) if n > 0 else d
        out["limiters_active_fraction_of_samples"] = active
        out["throttle_reason"] = (max(active, key=active.get) if active else "none reported (no accumulator advanced)")
        if "energy_J" in self.after and "energy_J" in self.before and frames > 0:
            out["joules_per_frame"] = round((self.after["energy_J"] - self.before["energy_J"]) / frames, 4)
            out["mean_socket_W_from_energy"] = round((self.after["energy_J"] - self.before["energy_J"]) / max(self.t_after - self.t_before, 1e-9), 1)
        out["limits_source"] = "amd-smi metric --throttle / --energy, before and after the sampled window (accumulators count SMU samples with the limiter active)"
        return out

    def summary(self):
        busy = [x for x in self.samples if x[1] > 400.0] or self.samples       # samples taken while the pipeline was loaded
        if not busy:
            return None
        clk, pw = sorted(x[0] for x in busy), sorted(x[1] for x in busy)
        return {"sclk_MHz_p50": clk[len(clk) // 2], "sclk_MHz_min": clk[0], "package_W_p50": pw[len(pw) // 2], "package_W_max": pw[-1],
                "samples": len(busy), "source": "rocm-smi --showclocks --showpower, polled during the timed regions (GPU 0)"}


def _power_cap_w():
    import re
    import subprocess
    try:
        out = subprocess.run(["rocm-smi", "--showmaxpower"], capture_output=True, text=True, timeout=5).stdout
        m = re.search(r"GPU\[0\]\s*:[^\n]*Power \(W\):\s*([0-9.]+)", out)
        return float(m.group(1)) if m else None
    except Exception:
        return None


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def roofline(det, pose, batch):
    """Dominant kernel = the conv_igemm instantiation with the largest summed device time; its achieved
    TFLOP/s = algorithmic FLOPs per launch / mean launch duration (HIP events around the kernel itself)."""
    groups = {}
    total_ms = 0.0
    for net in (det, pose):
        ms, info = net.profile(batch=batch, iters=10)
        flops, _bytes = net.op_stats()
        total_ms += float(ms.sum())
        carry_f = carry_b = 0.0          # FLOPs / bytes of convolutions computed inside the NEXT launch (members of a fused block: tile -1)
        for i in range(len(ms)):
            if not info[i, 0]:
                continue
            if int(info[i, 1]) == -1:
                carry_f += float(flops[i]) * batch
                carry_b += float(_bytes[i])
                continue
            key = (int(info[i, 1]), int(info[i, 2]))
            g = groups.setdefault(key, {"ms": 0.0, "flops": 0.0, "launches": 0, "bytes": 0.0})
            g["ms"] += float(ms[i])
            g["flops"] += float(flops[i]) * batch + carry_f
            g["bytes"] += float(_bytes[i]) + carry_b
            g["launches"] += 1
            carry_f = carry_b = 0.0
    key = max(groups, key=lambda k: groups[k]["ms"])
    g = groups[key]
    conv_ms = sum(v["ms"] for v in groups.values())
    conv_flops = sum(v["flops"] for v in groups.values())
    achieved = g["flops"] / (g["ms"] * 1e-3) / 1e12
    # HBM traffic per launch of that kernel: not measurable from inside the process -- taken from the committed
    # rocprofv3 PMC passes (profiles/*_pmc_traffic.json, collected with tools/pmc_traffic.sh, corrections inside)
    traffic, traffic_src, traffic_rw = None, None, None
    mode = {2: "f16", 3: "bf16x3"}.get(key[1], "f32")
    def kernel_name(tile, mode):
        if mode == "f32":
            return "bp::conv_igemm_kernel<%s, %d>" % (TILE_NAMES.get(tile, "?"), key[1])
        np_ = 1 if mode == "f16" else 3
        if tile in PL_TILE_ARGS:
            return "bp::conv_pl_kernel<%d, %s>" % (np_, PL_TILE_ARGS[tile][np_])
        if tile == 25:
            return "bp::conv_pl_kernel<1, 2, 2, 2, 2, 4, 1, 0, 1, false, *>"       # halo form of the 128x128 fp16 plane tile (* = halo rows, by map width)
        if tile == 12:
            return "bp::conv_igemm_h_kernel<1, 1, 3, true>"        # filters direct
        if tile in (21, 22):
            return "bp::conv_halo_kernel<%d, *>" % (2 if tile == 21 else 4)   # tap-resident halo (conv_halo.hip); * = loader passes, by map width
        if tile == 23:
            return "bp::conv_halo_k2_kernel<*>"                            # ... with two K groups inside the block
        if tile == 40:
            return "bp::conv_fused_kernel<*>"                              # whole residual / bottleneck block in one launch (conv_fused.hip)
        if tile == 26:
            return "bp::conv_s1_kernel<*>"                                 # 1x1 layers of the batched fp16 runs: persistent streaming kernel (conv_s1.hip; * = K chunks, K halves)
        if tile == 27:
            return "bp::conv_p3_kernel<*>"                                 # 3x3 / stride-1 layers of the batched fp16 runs: persistent kernel (conv_p3.hip; * = map width, halo rows, skip-connection format)
        if tile == 24:
            return "bp::conv_igemm_bdk2_kernel"                            # filters direct, two K groups inside an eight-wave block
        if tile in (7, 8, 9):
            return "bp::conv_kg_kernel<%d, 3>" % {7: 1, 8: 2, 9: 4}[tile]
        if tile in (10, 11):
            return "bp::conv_rd_kernel<%d>" % {10: 4, 11: 8}[tile]
        if tile >= 2:
            return "bp::conv_w64_kernel<%s, %d>" % (TILE_NAMES.get(tile, "?"), np_)
        return "bp::conv_igemm_h_kernel<%s, %d, false>" % (TILE_NAMES.get(tile, "?"), np_)
    name = kernel_name(key[0], mode)
    want = name.split(">")[0].split(", *")[0].split("<*")[0]
    peak_of = {"f32": PEAK_FP32_MFMA_TFLOPS, "f16": PEAK_F16_MFMA_TFLOPS, "bf16x3": PEAK_BF16X3_TFLOPS}
    per_kernel = []
    for k_, g_ in sorted(groups.items(), key=lambda kv: -kv[1]["ms"]):
        m_ = {2: "f16", 3: "bf16x3"}.get(k_[1], "f32")
        tf_ = g_["flops"] / (g_["ms"] * 1e-3) / 1e12
        per_kernel.append({"kernel": kernel_name(k_[0], m_) if m_ != "f32" else ("bp::stem3x3_kernel" if k_[0] == 20 else ("bp::stem7x7_f16_kernel" if k_[0] == 28 else "bp::conv_igemm_kernel<1, 1, %d>" % k_[1])),
                           "launches": g_["launches"], "us_per_step": round(g_["ms"] * 1e3, 1), "avg_launch_us": round(g_["ms"] / g_["launches"] * 1e3, 2),
                           "gflop": round(g_["flops"] / 1e9, 2), "achieved_TFLOPs": round(tf_, 1), "frac": round(tf_ / peak_of[m_], 4),
                           # (per-op bytes are the batch-1 figure -- fp32 operands and results, weights once: not scaled to batched runs)
                           "algorithmic_GBps": round(g_["bytes"] / (g_["ms"] * 1e-3) / 1e9, 1) if batch == 1 else None})
    try:
        import glob
        for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic*.json")))[::-1]:
            t = json.load(open(f))
            if t.get("kernel", "").startswith(want):
                traffic, traffic_src = t["traffic_bytes_per_launch"], os.path.relpath(f, ROOT)
                traffic_rw = {"fetch": t.get("fetch_bytes_per_launch"), "write": t.get("write_bytes_per_launch")}
                break
    except Exception:
        pass
    peak = {"f32": PEAK_FP32_MFMA_TFLOPS, "f16": PEAK_F16_MFMA_TFLOPS, "bf16x3": PEAK_BF16X3_TFLOPS}[mode]
    extra = {}
    if mode == "bf16x3":
        # six bf16 partial products per algorithmic multiply: the matrix cores execute 6x the algorithmic FLOPs;
        # "peak" is the algorithmic roof 2500 / 6 TFLOP/s
        extra = {"mfma_flops_per_algorithmic_flop": 6, "peak_executed_mfma": PEAK_F16_MFMA_TFLOPS}
    return {
        "bound": "mfma", "peak": round(peak, 1), "unit": "TFLOP/s",
        "traffic": traffic, "traffic_source": traffic_src,
        "traffic_fetch_write_bytes_per_launch": traffic_rw,     # (HBM-side bytes of the dominant kernel per launch, the two PMC passes apart)
        "algorithmic_bytes_per_launch": g["bytes"] / g["launches"],
        "kernel": name, "launches_per_step": g["launches"], "flops_per_launch": g["flops"] / g["launches"],
        # the dominant kernel ALONE (eager pass, hipExtLaunchKernelGGL start/stop events around every launch): its
        # launches never overlap here, so launches x duration exceeds ms_per_step of the multi-stream timed region
        "isolated": {"avg_launch_us": round(g["ms"] / g["launches"] * 1e3, 2), "achieved": round(achieved, 2),
                     "frac": round(achieved / peak, 4),
                     "all_conv": {"achieved": round(conv_flops / (conv_ms * 1e-3) / 1e12, 2), "ms_per_step": round(conv_ms, 4)},
                     "device_ms_per_step_eager_sum": round(total_ms, 4)},
        "kernels": per_kernel,
        "gflop_per_step": round(conv_flops / 1e9, 2), **extra,
        "layer_classes": layer_classes(det, pose, batch, peak),
        "algorithmic_bytes_per_step": sum(float(n_.op_stats()[1].sum()) for n_ in (det, pose)),
    }


def op_class(name: str, is_conv: bool) -> str:
    """The layer classes of the roofline table.  ``name`` = "<layer> k<ksize> <OH>x<OW> <Cin>-><Cout> s<stride>" for convs."""
    import re
    if not is_conv:
        return "se (pool + fc)" if ".se." in name else "other (max-pool, shuffle)"
    m = re.search(r" k(\d+) (\d+)x(\d+) (\d+)->(\d+) s(\d+)$", name)
    k, oh, ow, cin, cout = (int(m.group(i)) for i in range(1, 6))
    if cin <= 4:
        return "stems (RGB input, fp32 MFMA)"
    if cout < 64:
        return "heads (YOLO 1x1 -> 18, conv_out 3x3 -> 50)"
    if oh * ow <= 320:
        return "13x13 / 10x8 / 20x16 weight-bound (M <= 320)"
    return "3x3 mid (M > 320)" if k == 3 else "1x1 (M > 320)"


def layer_classes(det, pose, batch, peak_mode):
    """Per layer class, from the eager pass (every op alone between HIP events): launches, device time, achieved TFLOP/s
    against the MFMA roof of the class's arithmetic and ALGORITHMIC bytes (fp32 operands and results, weights
    once per launch) per second against the 8 TB/s HBM peak."""
    cls = {}
    for net in (det, pose):
        ms, info = net.profile(batch=batch, iters=10)
        flops, byts = net.op_stats()
        carry_g = carry_m = 0.0
        for i, (nm, is_conv) in enumerate(net.op_names()):
            fused_head = is_conv and int(info[i][1]) == 40
            c = cls.setdefault("fused blocks (1x1 -> 3x3 [-> 1x1] + skip, one launch)" if fused_head else op_class(nm, is_conv),
                               {"launches": 0, "ms": 0.0, "gflop": 0.0, "MB": 0.0})
            if int(info[i][1]) == -1:       # launches nothing: the op rides in its producer's epilogue (SE average pools) or inside the next launch (fused blocks)
                if is_conv:
                    carry_g += float(flops[i]) * batch / 1e9
                    carry_m += float(byts[i]) / 1e6
                continue
            c["launches"] += 1
            c["ms"] += float(ms[i])
            c["gflop"] += float(flops[i]) * batch / 1e9 + (carry_g if is_conv else 0.0)
            c["MB"] += float(byts[i]) / 1e6 + (carry_m if is_conv else 0.0)
            if is_conv:
                carry_g = carry_m = 0.0
    out = {}
    for k, c in sorted(cls.items(), key=lambda kv: -kv[1]["ms"]):
        pk = PEAK_FP32_MFMA_TFLOPS if k.startswith("stems") else peak_mode
        tf = c["gflop"] / c["ms"] if c["ms"] > 0 else 0.0          # GFLOP / ms = TFLOP/s
        gbps = c["MB"] / c["ms"] if c["ms"] > 0 else 0.0           # MB / ms = GB/s
        out[k] = {"launches": c["launches"], "us_per_step": round(c["ms"] * 1e3, 1), "gflop": round(c["gflop"], 2),
                  "achieved_TFLOPs": round(tf, 1), "mfma_frac": round(tf / pk, 4) if c["gflop"] > 0 else None,
                  "algorithmic_GBps": round(gbps, 1), "hbm_frac": round(gbps / PEAK_HBM_GBPS, 4)}
    return out


def mode_bytes_per_frame(nets, batch: int, elem_bytes: float) -> float:
    """Algorithmic HBM bytes per frame OF THE MODE THAT RAN at `batch` frames per launch: every convolution's input, output and skip
    connection at `elem_bytes` per element (2 = the fp16 operand planes the fp16 modes move), its filters at `elem_bytes` per element ONCE
    per launch (so 1/batch per frame); non-convolution ops keep their fp32 byte counts.  (op_stats' own figure is SURVEY 8(d)'s: fp32
    operands and results, weights once per FRAME -- the right denominator at batch 1 in the fp32-accurate mode only.)"""
    import re
    total = 0.0
    for net in nets:
        _f, byts = net.op_stats()
        for i, (nm, is_conv) in enumerate(net.op_names()):
            b = float(byts[i])
            if not is_conv:
                total += b
                continue
            m = re.search(r" k(\d+) (\d+)x(\d+) (\d+)->(\d+) s(\d+)$", nm)
            k, cin, cout = int(m.group(1)), int(m.group(4)), int(m.group(5))
            w = float(k * k * cin * cout)
            total += (b / 4.0 - w) * elem_bytes + w * elem_bytes / batch
    return total


def hbm_block(alg_bytes_per_step: float, fps: float, batch: int, precision: str = "bf16x3", suffix=None):
    """HBM GB/s of the whole pipeline at the measured rate: counter bytes per frame from the committed rocprofv3 PMC pass
    (tools/pmc_frame_traffic.sh: FETCH_SIZE x 2 on gfx950 + WRITE_SIZE, separate passes) x frames/s, beside the algorithmic
    bytes per frame x frames/s."""
    src, counter = None, None
    try:
        import glob
        suffix = suffix if suffix is not None else {"bf16x3": "", "f16": "_f16", "f16r": "_f16", "f32": "_f32"}[precision]
        for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_frame_traffic%s.json" % suffix)))[::-1]:
            t = json.load(open(f))
            counter = (t["fetch_MB_per_frame(x2 corrected)"] + t["write_MB_per_frame"]) * 1e6
            src = os.path.relpath(f, ROOT)
            break
    except Exception:
        pass
    alg = alg_bytes_per_step / batch
    return {"achieved_GBps": round(counter * fps / 1e9, 1) if counter else None,
            "algorithmic_GBps": round(alg * fps / 1e9, 1), "peak": PEAK_HBM_GBPS,
            "frac": round(counter * fps / 1e9 / PEAK_HBM_GBPS, 4) if counter else None,
            "counter_bytes_per_frame": counter, "algorithmic_bytes_per_frame": alg,
            "traffic_over_algorithmic": round(counter / alg, 2) if counter else None, "source": src,
            "note": "achieved = HBM-side bytes per frame (PMC, fetch doubled per MI355X_MICROARCH.md) x the frames/s of this run"}


def insitu_layers(dets, poses, run, S, batch, path, precision):
    """Per-layer timing WHILE the pipeline runs (S frames in flight, graph replay): every conv kernel stamps s_memrealtime (the device-wide
    100 MHz reference clock) at its blocks' entry, K-loop end and last store (bp_*_set_stamps); a layer's span = first entry -> last mark of its grid.
    rocprofv3 cannot give this (its tracer serialises the streams).  Writes the table to ``path``."""
    import ctypes
    import torch
    from betapose_amd import _lib
    SLOTS = 4096
    nets = []
    for k in range(S):
        for tag, net in (("yolo", dets[k]), ("kpd", poses[k])):
            names = net.op_names()
            nconv = sum(1 for _, c in names if c)
            buf = torch.zeros(nconv * SLOTS * 8, dtype=torch.int64, device="cuda")
            net.set_stamps(buf, SLOTS)
            nets.append((k, tag, net, [n for n, c in names if c], buf))
    run(2 * S, False)                 # graphs re-captured with the stamp pointers, pipeline warm
    torch.cuda.synchronize()
    for *_, buf in nets:
        buf.zero_()
    n = 6 * S
    t0 = time.perf_counter()
    run(n, False)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    ms = ctypes.c_float(0)
    TICKS = 2_000_000                 # 20 ms of the 100 MHz reference clock the stamps read
    _lib.check(_lib.lib().bp_calibrate_ticks(TICKS, ctypes.byref(ms), _lib.current_stream()))
    ghz = TICKS / (ms.value * 1e-3) / 1e9
    rows, spans, dumps = [], [], []
    for k, tag, net, names, buf in nets:
        a = buf.cpu().numpy().reshape(len(names), SLOTS, 8)
        for c, nm in enumerate(names):
            blk = a[c][a[c, :, 0] != 0]
            if not len(blk):
                rows.append((k, tag, c, nm, 0, None))
                continue
            entry = blk[:, 0]
            last = blk[:, 3:7].max(axis=1)
            if os.environ.get("BP_INSITU_DUMP") and os.environ["BP_INSITU_DUMP"] in nm and k == 0:
                # per-block marks of one layer (10-ns ticks since the layer's first entry): entry | K loop done | last mark
                e0_ = int(entry.min())
                order = np.argsort(entry)
                dumps.append("# blocks of %s (stream 0), sorted by entry: entry kloop_done last [us]\n" % nm + "\n".join(
                    "#   %7.2f %7.2f %7.2f" % ((entry[i] - e0_) / 100.0, (blk[i, 3] - e0_) / 100.0 if blk[i, 3] else -1, (last[i] - e0_) / 100.0) for i in order))
            kloop = (blk[:, 3] - blk[:, 0])[blk[:, 3] != 0]
            rows.append((k, tag, c, nm, len(blk), (int(entry.min()), int(last.max()), float(kloop.mean()) if len(kloop) else 0.0,
                                                    float((last - np.maximum(blk[:, 3], entry)).mean()))))
            spans.append((int(entry.min()), int(last.max())))
        net.set_stamps(None, 0)
    us = lambda t: t / ghz / 1e3
    # where every stream's last frame was in time: first stamped entry of its YOLO and the last mark of its KPD
    phase = {}
    for k, tag, c, nm, nb, r in rows:
        if r is not None:
            ph = phase.setdefault(k, [r[0], r[1]])
            ph[0], ph[1] = min(ph[0], r[0]), max(ph[1], r[1])
    t_first = min(v[0] for v in phase.values()) if phase else 0
    stream_phase = {str(k): {"start_us": round(us(v[0] - t_first), 1), "frame_us": round(us(v[1] - v[0]), 1)} for k, v in sorted(phase.items())}
    # layers in flight at once over the stamped window (the last frame of each stream): sum of spans / union of spans
    ev = sorted([(s0, 1) for s0, _ in spans] + [(s1, -1) for _, s1 in spans])
    busy = depth = 0
    prev = ev[0][0]
    for t, d in ev:
        if depth > 0:
            busy += t - prev
        depth += d
        prev = t
    conc = sum(s1 - s0 for s0, s1 in spans) / max(busy, 1)
    per_class, lines = {}, []
    for k, tag, c, nm, nb, r in rows:
        if r is None:
            lines.append("%d %-4s %3d %-58s no stamps (grid > %d blocks)" % (k, tag, c, nm, SLOTS))
            continue
        e0, e1, kl, tail = r
        lines.append("%d %-4s %3d %-58s blocks %5d  span %7.2f us  K loop (mean per block) %7.2f us  tail %6.2f us" % (
            k, tag, c, nm, nb, us(e1 - e0), us(kl), us(tail)))
        pc = per_class.setdefault(op_class(nm, True), {"launches": 0, "span_us": 0.0, "kloop_us": 0.0})
        pc["launches"] += 1
        pc["span_us"] += us(e1 - e0)
        pc["kloop_us"] += us(kl)
    for v in per_class.values():
        v["launches"] //= S
        v["span_us"] = round(v["span_us"] / S, 1)
        v["kloop_us"] = round(v["kloop_us"] / S, 1)
    summary = {"frames_in_flight": S, "stamp_clock_GHz": round(ghz, 3), "mean_layers_in_flight": round(conc, 2),
               "per_class_us_per_frame": per_class, "last_frame_of_each_stream": stream_phase, "table": os.path.relpath(path, ROOT) if path.startswith(ROOT) else path,
               "fps_while_stamping": round(n * batch / (wall_ms * 1e-3), 1)}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# in-situ per-layer times: %d frames in flight, precision %s, the LAST frame of every stream; clock %.3f GHz\n"
                "# (bench.py --insitu; stamps = s_memrealtime written by the conv kernels: entry / K loop done / last store per block)\n"
                "# span = first block entry -> last mark of the layer's grid; %.2f layers in flight on average\n" % (S, precision, ghz, conc))
        f.write("# stream net conv layer\n" + "\n".join(lines) + "\n" + "".join(d + "\n" for d in dumps) + "# " + json.dumps(summary) + "\n")
    return summary


def served_leg(ys, ks, local, batch, streams, precision, steps, kp3d, cam_K, label, detail=False, power=False):
    """One more line of the same hot path with `batch` frames per launch on `n_streams` streams (the reference's --detbatch,
    dataloader.py:284-289): its own engines (max_batch = batch), frames resident in HBM, host tail inside the timed region,
    barrier-free single-GPU timing (synchronize both sides).  Returns frames/s, ms per step and the convolution GFLOP per frame."""
    import torch
    from betapose_amd.darknet import Darknet
    from betapose_amd.kpd import FastPoseHIP
    from betapose_amd.pipeline import FramePipeline, finish_record
    from betapose_amd import synth
    dev = torch.device("cuda", local)
    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416, max_batch=batch, device=local)
    det.load_stream(ys)
    pose = FastPoseHIP.from_stream(ks, n_classes=50, max_batch=batch, device=local)
    det.cuda(); pose.cuda()
    det.set_precision(precision); pose.set_precision(precision)
    # the HIP streams of the main run are reused: streams created now would share hardware queues unevenly with them (the runtime
    # maps streams onto 4 queues round robin; measured here: 686 instead of 1 110 frames/s at 2 x 4 with fresh streams)
    S = len(streams)
    dets = [det] + [det.clone() for _ in range(S - 1)]
    poses = [pose] + [pose.clone() for _ in range(S - 1)]
    pipes = [FramePipeline(dets[k], poses[k], 480, 640, batch=batch, confidence=0.01, num_classes=80, use_graph=True) for k in range(S)]
    pool = [torch.from_numpy(np.stack(synth.synth_frames(batch, 4321 + 37 * j))).to(dev) for j in range(4)]
    NS = 2 * S
    pinned = [torch.empty((batch, pipes[0].results.shape[1]), dtype=torch.float32).pin_memory() for _ in range(NS)]
    events = [torch.cuda.Event() for _ in range(NS)]
    got = {"poses": 0}

    def issue(i):
        k = i % S
        with torch.cuda.stream(streams[k]):
            pipes[k].frames.copy_(pool[i % len(pool)], non_blocking=True)
            pipes[k].enqueue(streams[k].cuda_stream)
            pinned[i % NS].copy_(pipes[k].results, non_blocking=True)
            events[i % NS].record(streams[k])

    def finish(i):
        events[i % NS].synchronize()
        rec = pinned[i % NS].numpy()
        for b in range(batch):
            got["poses"] += len(finish_record(rec[b], "%06d.png" % (i * batch + b), kp3d, cam_K)["result"]) > 0

    def run(n):
        for i in range(n):
            issue(i)
            if i >= S:
                finish(i - S)
        for i in range(max(0, n - S), n):
            finish(i)

    run(max(2 * S, 8))                       # graphs captured, buffers touched
    torch.cuda.synchronize()
    tw = time.perf_counter()
    run(max(2 * S, 8))                       # warm, and the step time the timed region is sized from (>= `steps`, >= ~1.5 s)
    torch.cuda.synchronize()
    tw = (time.perf_counter() - tw) / max(2 * S, 8)
    steps = int(min(max(steps, 1.5 / max(tw, 1e-6)), 4000))
    cs = ClockSampler(period=0.25) if power else None
    if cs:
        cs.__enter__()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if cs:
        cs.__exit__(None, None, None)
    gflop = sum(float(n_.op_stats()[0].sum()) for n_ in (det, pose)) / 1e9          # conv FLOPs per frame (op_stats is per image)
    alg_bytes = sum(float(n_.op_stats()[1].sum()) for n_ in (det, pose))
    if precision in ("f16", "f16r"):   # the bytes of the mode that ran: fp16 planes, filters once per launch
        alg_bytes = mode_bytes_per_frame((det, pose), batch, 2.0)
    res = {"label": label, "value": round(steps * batch / el, 2), "unit": "frames/sec", "batch": batch, "streams": S, "precision": precision,
           "steps": steps, "ms_per_step": round(el / steps * 1e3, 4), "poses": got["poses"], "graph_nodes": pipes[0].kernel_count()}
    if cs:       # shader clock / socket power / SMU limiter / joules per frame DURING this leg's timed region (round 6: the batched fp16 legs sit on
        # the socket power cap -- frames/s there is 1 / joules per frame)
        pw = dict(cs.summary() or {})
        pw.update(cs.limits(steps * batch) or {})
        pw["power_cap_W"] = _power_cap_w()
        res["power"] = pw
    if detail:   # the leg's own kernel table and layer classes (eager pass, every launch alone between HIP events) at ITS batch size and precision
        rf = roofline(det, pose, batch)
        res["detail"] = {"kernels": rf["kernels"], "isolated": rf["isolated"], "layer_classes": rf["layer_classes"]}
    del pipes, dets, poses, det, pose
    torch.cuda.synchronize()
    return res, gflop, alg_bytes


def dump_outputs(path, recs, outs):
    """--dump-outputs: what a caller of the timed path receives for the frames of one step, as float32 / float64 .npy files.
    `recs` [batch, 316] are the device records; their int32 fields (detector index, key-point arg-max pixel) are written as
    their integer values in float64, not as the bits.  `outs` are finish_record's dicts; NaN where a frame has no detection
    or no pose."""
    os.makedirs(path, exist_ok=True)
    recs = np.ascontiguousarray(recs, dtype=np.float32)
    r64 = recs.astype(np.float64)
    ints = [0] + list(range(16, recs.shape[1], 6))
    r64[:, ints] = recs[:, ints].view(np.int32)
    n = len(outs)
    arrays = {"records": r64, "boxes": np.full((n, 4), np.nan, np.float32), "box_scores": np.full((n,), np.nan, np.float32),
              "keypoints": np.full((n, 50, 2), np.nan, np.float32), "kp_scores": np.full((n, 50), np.nan, np.float32),
              "proposal_scores": np.full((n,), np.nan, np.float32),
              "cam_R": np.full((n, 3, 3), np.nan, np.float64), "cam_t": np.full((n, 3), np.nan, np.float64)}
    for b, o in enumerate(outs):
        if o.get("boxes") is not None:
            arrays["boxes"][b] = np.asarray(o["boxes"]).reshape(4)
            arrays["box_scores"][b] = np.asarray(o["scores"]).reshape(-1)[0]
        if o["result"]:
            r = o["result"][0]
            arrays["keypoints"][b] = np.asarray(r["keypoints"]).reshape(50, 2)
            arrays["kp_scores"][b] = np.asarray(r["kp_score"]).reshape(50)
            arrays["proposal_scores"][b] = np.asarray(r["proposal_score"]).reshape(-1)[0]
        if len(o["cam_R"]):
            arrays["cam_R"][b] = np.asarray(o["cam_R"]).reshape(3, 3)
            arrays["cam_t"][b] = np.asarray(o["cam_t"]).reshape(3)
    for name, arr in arrays.items():
        np.save(os.path.join(path, name + ".npy"), arr)


def main():
    a = parse_args()
    import torch
    from betapose_amd import _lib, cfg as C, dist as bpd, synth
    from betapose_amd.darknet import Darknet
    from betapose_amd.kpd import FastPoseHIP
    from betapose_amd.pipeline import FramePipeline, finish_record
    from betapose_amd.weights import fastpose_stream_from_state_dict

    _lib.require_gpu()
    bpd.limit_host_threads()
    rank, world, local = bpd.init_from_env()
    dev = torch.device("cuda", local)

    # ---- weights: rank 0 builds the two fp32 streams, everyone else receives them over RCCL
    blocks = C.parse_cfg_text(C.yolov3_single_cfg_text())
    ys = ks = None
    if rank == 0:
        ys = synth.synth_yolo_stream(1, blocks)
        ks = fastpose_stream_from_state_dict(synth.synth_fastpose_state_dict(2))
    t_bc = time.perf_counter()
    ys, ks = bpd.broadcast_stream(ys), bpd.broadcast_stream(ks)
    if world > 1:
        torch.cuda.synchronize()
    t_bc = (time.perf_counter() - t_bc) * 1e3
    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416, max_batch=a.batch, device=local)
    det.load_stream(ys)
    pose = FastPoseHIP.from_stream(ks, n_classes=50, max_batch=a.batch, device=local)
    det.cuda()
    pose.cuda()

    det.set_policy(a.sk_target, a.sk_min, a.sk_max, a.tile)
    pose.set_policy(a.sk_target, a.sk_min, a.sk_max, a.tile)
    det.set_precision(a.precision)       # clones made below inherit it
    pose.set_precision(a.precision)
    S = max(1, a.streams)
    dets = [det] + [det.clone() for _ in range(S - 1)]
    poses = [pose] + [pose.clone() for _ in range(S - 1)]
    for d, p_ in zip(dets[1:], poses[1:]):
        d.set_policy(a.sk_target, a.sk_min, a.sk_max, a.tile)
        p_.set_policy(a.sk_target, a.sk_min, a.sk_max, a.tile)
    if a.prefetch:
        for d, p_ in zip(dets, poses):
            d.set_prefetch(True)
            p_.set_prefetch(True)
    pipes = [FramePipeline(dets[k], poses[k], 480, 640, batch=a.batch, confidence=0.01, num_classes=80,
                           use_graph=not a.no_graph) for k in range(S)]
    masked = []
    if a.partition:
        from betapose_amd.streams import MaskedStream, partition_cus
        slices = partition_cus(a.partition)
        masked = [MaskedStream(*slices[k % len(slices)], device=local) for k in range(S)]
        streams = [m.torch for m in masked]
    else:
        streams = [torch.cuda.Stream(device=dev) for _ in range(S)]
    pipe = pipes[0]
    if a.fixed_box:
        for p_ in pipes:
            p_.set_fixed_box([220, 140, 420, 340])
    # (FramePipeline.prepare() -- graph capture as a set-up step -- is NOT used here: it buys the first region nothing (measured) and, called
    # before the streams' first launches, it left two frames in flight on ONE hardware queue: 392 against 659 frames/s at --streams 2)
    kp3d, cam_K = synth.synth_kp3d(50), synth.CAM_K

    # ---- inputs resident in HBM: a pool of distinct frames per rank
    pool_host = [torch.from_numpy(np.stack(synth.synth_frames(a.batch, 1234 + 1000 * rank + 37 * j))).pin_memory()
                 for j in range(a.pool)]
    pool = [f.to(dev) for f in pool_host]
    NS = 2 * S
    pinned = [torch.empty((a.batch, pipe.results.shape[1]), dtype=torch.float32).pin_memory() for _ in range(NS)]
    events = [torch.cuda.Event() for _ in range(NS)]
    records = np.zeros((a.steps, a.batch, pipe.results.shape[1]), np.float32)
    last_outs = []                 # finish_record's dicts of the last timed step (--dump-outputs)
    stats = {"det": 0, "pose": 0}
    t_issue = np.zeros(max(a.steps, 1))
    lat = {"on": False, "ms": []}
    src = {"pool": pool}           # frames resident in HBM (the headline) or pinned host memory (h2d_inclusive)
    torch.cuda.synchronize()

    def issue(i):
        k = i % S
        if lat["on"]:
            t_issue[i] = time.perf_counter()
        with torch.cuda.stream(streams[k]):
            pipes[k].frames.copy_(src["pool"][i % a.pool], non_blocking=True)
            pipes[k].enqueue(streams[k].cuda_stream)
            pinned[i % NS].copy_(pipes[k].results, non_blocking=True)
            events[i % NS].record(streams[k])

    def finish(i, keep):
        events[i % NS].synchronize()
        if lat["on"]:
            lat["ms"].append((time.perf_counter() - t_issue[i]) * 1e3)     # frame handed over -> record on the host
        rec = pinned[i % NS].numpy()
        for b in range(a.batch):
            out = finish_record(rec[b], "%06d.png" % (i * a.batch + b), kp3d, cam_K)
            if keep:
                stats["det"] += out.get("boxes") is not None
                stats["pose"] += len(out["result"]) > 0
                if i == a.steps - 1:
                    last_outs.append(out)
        if keep:
            records[i] = rec

    def run(nsteps, keep, depth=None):
        d = S if depth is None else depth          # frames left in flight behind the one just issued (0: one at a time)
        for i in range(nsteps):
            issue(i)
            if i >= d:
                finish(i - d, keep)
        for i in range(max(0, nsteps - d), nsteps):
            finish(i, keep)

    # exactly the W warm-up steps asked for (round 4; rounds 2-3 ran at least 60): `value` is the K-step region right behind
    # them.  The device's clock / power state and the streams' stagger settle over ~60 frames (K = 20, one box: 902-912
    # frames/s after 5 warm-up steps, 933-938 after 60) -- that figure is reported beside it as `value_settled`
    warmup_run = max(a.warmup, 1)
    run(warmup_run, False)
    torch.cuda.synchronize()
    bpd.barrier()
    torch.cuda.synchronize()
    lat["on"] = True
    t0 = time.perf_counter()
    cpu0 = time.process_time()
    run(a.steps, True)
    t_own = time.perf_counter() - t0
    cpu_own = time.process_time() - cpu0      # host CPU seconds of this rank (all its threads) inside the timed region
    lat["on"] = False
    # xGMI gather of detections only: steps*batch records of 316 floats per rank, in global frame order on rank 0
    flat = records.reshape(-1, records.shape[-1])
    gathered = bpd.gather_records(flat, [rank + world * j for j in range(len(flat))], world * len(flat))
    torch.cuda.synchronize()
    bpd.barrier()
    torch.cuda.synchronize()
    el = bpd.max_over_ranks(time.perf_counter() - t0)
    lat_flight = np.array(lat["ms"]) if lat["ms"] else np.zeros(1)
    rank_fps = bpd.gather_floats(a.steps * a.batch / t_own)
    rank_cpu_ms = bpd.gather_floats(cpu_own / (a.steps * a.batch) * 1e3)
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, records[-1], last_outs)

    # ---- more K-step regions, back to back, each bracketed like the first (barrier + synchronize both sides, max over
    # ranks): a single 20-step region is a 20 ms window
    region_fps = [world * a.steps * a.batch / el]
    # regions that START after >= 60 frames have run are "settled"; at least three of those (short regions: a few more)
    frames_before = [warmup_run * a.batch]
    n_regions = max(1, a.repeats)
    while a.repeats > 1 and sum(1 for i in range(n_regions) if (warmup_run + i * a.steps) * a.batch >= 60) < 3 and n_regions < 16:
        n_regions += 1
    for _ in range(n_regions - 1):
        frames_before.append(frames_before[-1] + a.steps * a.batch)
        torch.cuda.synchronize()
        bpd.barrier()
        torch.cuda.synchronize()
        tr = time.perf_counter()
        run(a.steps, False)
        torch.cuda.synchronize()
        bpd.barrier()
        torch.cuda.synchronize()
        region_fps.append(world * a.steps * a.batch / bpd.max_over_ranks(time.perf_counter() - tr))

    # ---- side measurements on the same pipelines (never `value`): strictly one frame at a time, and the same
    # multi-frame run with every frame uploaded from pinned host memory inside the timed region
    side = {}
    if a.full and world == 1 and not a.no_side_runs:
        n1 = min(a.steps, 100)

        def one_at_a_time(prefetch):
            for d, p_ in zip(dets, poses):        # lone-frame latency mode: XCD-matched layout + next-layer filter prefetch
                d.set_prefetch(prefetch)
                p_.set_prefetch(prefetch)
            run(2 * S, False, depth=0)            # (re-captures every stream's graph)
            torch.cuda.synchronize()
            lat["ms"], lat["on"] = [], True
            t1 = time.perf_counter()
            run(n1, False, depth=0)
            torch.cuda.synchronize()
            t1 = time.perf_counter() - t1
            lat["on"] = False
            one = np.array(lat["ms"])
            r_ = {"p50": round(float(np.percentile(one, 50)), 4), "p95": round(float(np.percentile(one, 95)), 4),
                  "frames_per_sec": round(n1 * a.batch / t1, 2)}
            if prefetch:   # the mode's placement check (an error word since round 5, not a trap): must be 0 for the figure to count
                # (bp_pipeline_run reads and clears the engines' error words itself in this mode and re-runs a faulted frame: count those)
                r_["xcd_placement_errors"] = int(sum(pp.latency_faults() for pp in pipes))
            return r_

        side["single"] = one_at_a_time(True)
        side["single"]["filter_prefetch"] = True
        side["single"]["without_filter_prefetch"] = one_at_a_time(a.prefetch)
        if a.prefetch:
            side["single"].pop("without_filter_prefetch")
        # shader clock and package power under this pipeline's load: ~4 s of the same multi-frame run, sampled
        with ClockSampler() as cs:
            t_c = time.perf_counter()
            n_c = 0
            while time.perf_counter() - t_c < 4.0:
                run(max(4 * S, 50), False)
                n_c += max(4 * S, 50)
            torch.cuda.synchronize()
            t_c = time.perf_counter() - t_c
        if cs.summary():
            side["clocks"] = dict(cs.summary(), frames_per_sec_meanwhile=round(n_c * a.batch / t_c, 1))
            lim = cs.limits(n_c * a.batch)
            if lim:
                side["clocks"]["power_cap_W"] = _power_cap_w()
                side["clocks"].update(lim)
        src["pool"] = pool_host
        n2 = min(a.steps, 200)
        run(2 * S, False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        run(n2, False)
        torch.cuda.synchronize()
        t2 = time.perf_counter() - t2
        src["pool"] = pool
        side["h2d"] = {"value": round(n2 * a.batch / t2, 2), "unit": "frames/sec", "steps": n2,
                       "ms_per_step": round(t2 / n2 * 1e3, 4),
                       "note": "every step uploads its %d-byte frame from pinned host memory (hipMemcpyAsync on the "
                               "frame's stream) inside the timed region" % (a.batch * 480 * 640 * 3)}

    out = None
    if rank == 0:
        frames_total = world * a.steps * a.batch
        out = {
            "metric": "frames/sec (640x480, 50-kp KPD)", "value": round(frames_total / el, 2), "unit": "frames/sec",
            # protocol 2 (round 4 on): exactly --warmup steps, `value` = the K-step region right behind them.  Rounds 2-3 (protocol 1)
            # forced >= 60 warm-up frames, so their `value` compares with this line's `value_settled`, not with `value`.
            "protocol_version": 2,
            "value_definition": "K timed steps right behind exactly W warm-up steps, frames RESIDENT IN HBM when the timed region starts (the "
                                "bench contract of this tier: the PCIe-inclusive rate is never `value`; SURVEY 8(d)'s upload-inclusive figure is "
                                "`h2d_inclusive` beside it under --full, within noise of `value`); compare across rounds on `value_settled` (--full)",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "warmup_steps_run": warmup_run, "ms_per_step": round(el / a.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"f32": "f32", "f16": "f16 MFMA operands, f32 accumulate and activations",
                      "f16r": "f16 MFMA operands, f32 accumulate, fp16 skip connections (residuals read from the fp16 operand planes)",
                      "bf16x3": "f32 as an exact 3-way bf16 operand split (6 bf16 MFMA products), f32 accumulate and "
                                "activations"}[a.precision],
            "data": "synthetic (seeded 640x480 BGR u8 frames resident in HBM; seeded random weights of the "
                    "reference architectures)",
            "config": {"workload": "BASELINE configs[1]: single-object frame, YOLOv3 416x416 (1 class) -> 1 crop "
                                   "320x256 -> FastPose SE-ResNet-101+DUC (the reference's real KPD, SURVEY F1) -> "
                                   "50 kp arg-max -> pPose-NMS -> PnP",
                       "batch": a.batch, "global_batch": a.batch * world, "frame": "640x480x3 u8",
                       "parallelism": "frames sharded by image, 1 process per GPU (dp%d)" % world,
                       "hip_graph": not a.no_graph, "fixed_box": a.fixed_box, "frames_in_flight": S, "cu_partition": a.partition,
                       "graph_nodes": pipe.kernel_count()},
            "latency_ms": {"frames_in_flight": S, "p50": round(float(np.percentile(lat_flight, 50)), 4),
                           "p95": round(float(np.percentile(lat_flight, 95)), 4),
                           "definition": "frame handed to the stream -> its record (post-processing input) on the host",
                           **({"one_frame_at_a_time": side["single"]} if "single" in side else {})},
            **({"clocks_under_load": side["clocks"]} if "clocks" in side else {}),
            "detections": stats["det"], "poses": stats["pose"],
            "host_cpu_ms_per_frame": round(rank_cpu_ms[0], 3),
            "records_gathered": int((gathered[:, 0].view(np.int32) >= -1).sum()) if gathered is not None else 0,
        }
        assert gathered.shape == (frames_total, records.shape[-1])
        if a.full:
            out["value_settled"] = round(float(np.percentile([v for v, fb in zip(region_fps, frames_before) if fb >= 60] or region_fps, 50)), 2)
            out["repeats"] = {"regions": len(region_fps), "steps_each": a.steps, "fps": [round(v, 2) for v in region_fps],
                              "p50": round(float(np.percentile(region_fps, 50)), 2), "min": round(min(region_fps), 2),
                              "max": round(max(region_fps), 2), "frames_run_before_each": frames_before,
                              "note": "`value` is region 0 (right behind the commanded warm-up); `value_settled` = p50 of the regions that started after >= 60 frames"}
            t1 = time.perf_counter()
            for _ in range(200):
                finish_record(records[0, 0], "x.png", kp3d, cam_K)
            out["host_post_ms_per_frame"] = round((time.perf_counter() - t1) / 200 * 1e3, 4)
        if "h2d" in side:
            out["h2d_inclusive"] = side["h2d"]
        if world > 1:
            import torch.distributed as tdist
            out["rccl"] = {"backend": tdist.get_backend(), "ranks": world, "weight_broadcast_ms": round(t_bc, 1),
                           "per_rank_frames_per_sec": [round(v, 2) for v in rank_fps],
                           "per_rank_host_cpu_ms_per_frame": [round(v, 3) for v in rank_cpu_ms],
                           "host_cores": os.cpu_count(),
                           "collectives": "broadcast of 2 fp32 weight streams (246 + 239 MB) at start-up, all_gather of "
                                          "316-float records, barriers around the timed region"}
    if a.full and rank == 0 and not a.no_roofline:
        rf = roofline(det, pose, a.batch)
        # IN-SITU figure = the convolution FLOPs of the timed steps over the wall clock of the timed region (all frames
        # in flight, per GPU): kernel time per step <= ms_per_step holds by construction
        agg = rf["gflop_per_step"] * a.steps / el / 1e3
        out["roofline"] = {"bound": rf["bound"], "achieved": round(agg, 2), "peak": rf["peak"], "unit": rf["unit"],
                           "frac": round(agg / rf["peak"], 4), "traffic": rf["traffic"],
                           # the per-kernel figure SURVEY 8(d) asks for, beside the pipeline aggregate above: the by-time-dominant kernel ALONE
                           # (algorithmic FLOPs per launch / its mean launch duration between HIP events) over the same roof
                           "dominant_kernel_frac": rf["isolated"]["frac"], "dominant_kernel_avg_launch_us": rf["isolated"]["avg_launch_us"],
                           "definition": "`achieved` / `frac` are the AGGREGATE of all frames in flight: algorithmic conv FLOPs of the timed steps / wall clock of the "
                                         "timed region, per GPU (several kernels run side by side); `dominant_kernel_frac` (= `isolated.frac`) is the "
                                         "kernel roofline: the dominant kernel's algorithmic FLOPs per launch / its average launch duration",
                           **{k: v for k, v in rf.items() if k not in ("bound", "peak", "unit", "traffic")}}
        if a.precision == "bf16x3":
            out["roofline"]["frac_of_executed_mfma"] = round(6 * agg / PEAK_F16_MFMA_TFLOPS, 4)
        out["roofline"]["hbm"] = hbm_block(rf["algorithmic_bytes_per_step"], out["value"] / world, a.batch, a.precision)
    if rank == 0 and world == 1 and a.insitu:
        out.setdefault("roofline", {})["insitu"] = insitu_layers(dets, poses, run, S, a.batch, a.insitu, a.precision)
    if a.full and rank == 0 and world == 1 and a.other_modes:
        # the opt-in precisions on the same workload, for the record: 4 frames in flight, same
        # graph pipeline (re-captured on the precision change), a short timed run each
        other = {}
        for mode in [m for m in a.other_modes.split(",") if m and m != a.precision]:
            for d, p_ in zip(dets, poses):
                d.set_precision(mode)
                p_.set_precision(mode)
            n_alt = min(a.steps, 120)
            run(max(2 * S, 8), False)
            torch.cuda.synchronize()
            t_alt = time.perf_counter()
            run(n_alt, False)
            torch.cuda.synchronize()
            other[mode] = {"value": round(n_alt * a.batch / (time.perf_counter() - t_alt), 2), "unit": "frames/sec",
                           "steps": n_alt}
        for d, p_ in zip(dets, poses):
            d.set_precision(a.precision)
            p_.set_precision(a.precision)
        other["note"] = ("bf16x3 = fp32-accurate (exact 3-way bf16 operand split, passes the whole parity suite); "
                         "f16 = fp16 operands (stated-tolerance mode, BASELINE configs[2])")
        out["other_precisions"] = other
    if a.full and rank == 0 and world == 1 and not a.no_served_legs and len(streams) >= 4 and not a.partition:
        # BASELINE configs[2] on the driver's clock: fp16 MFMA operands, 28 crops / frames per launch, 3 streams
        c2, gf, ab = served_leg(ys, ks, local, 28, streams[:3], "f16", max(30, min(a.steps, 60)), kp3d, cam_K,
                                "BASELINE configs[2]: batched inference, 28 frames per launch x 3 streams, fp16 MFMA conv path "
                                "(fp16 operands, fp32 accumulation, fp32 activations and skip connections)", detail=True, power=True)
        c2_detail = c2.pop("detail")
        # the same leg with fp16 skip connections ('f16r': residuals read from the fp16 operand planes, fp32 copies of block outputs
        # dropped -- a further stated-tolerance step, tests/test_gpu_nets.py::test_f16r_mode_fp16_skip_connections)
        c2r, _, _ = served_leg(ys, ks, local, 28, streams[:3], "f16r", max(30, min(a.steps, 60)), kp3d, cam_K,
                               "configs[2] with fp16 skip connections (precision 'f16r')", power=True)
        c2["with_fp16_skip_connections"] = {k_: c2r[k_] for k_ in ("label", "value", "unit", "steps", "ms_per_step", "precision", "power") if k_ in c2r}
        c2["with_fp16_skip_connections"]["roofline_frac"] = round(gf * c2r["value"] / 1e3 / PEAK_F16_MFMA_TFLOPS, 4)
        tf = gf * c2["value"] / 1e3
        c2["roofline"] = {"bound": "mfma", "achieved": round(tf, 1), "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_F16_MFMA_TFLOPS, 4),
                          "gflop_per_frame": round(gf, 2), "definition": "algorithmic conv FLOPs of the timed steps / wall clock, all streams",
                          # the leg's own kernels and layer classes, every launch alone between HIP events at 28 frames per launch (round-4 verdict item 4)
                          "kernels": c2_detail["kernels"], "isolated": c2_detail["isolated"], "layer_classes": c2_detail["layer_classes"],
                          # HBM side: counter bytes per frame (committed PMC pass of this leg) x frames/s against the 8 TB/s peak, beside the
                          # algorithmic bytes OF THE MODE THAT RAN (fp16 planes in and out, fp16 filters once per 28-frame launch; `ab`)
                          "hbm": dict(hbm_block(ab * 28, c2["value"], 28, "f16", "_batch28_f16"),
                                      algorithmic_definition="2 B per activation element read and written (fp16 operand planes, skip connections included), "
                                                             "fp16 filters once per 28-frame launch; fp32 for the non-convolution ops")}
        out["configs2"] = c2
        # served-stream lines of the default precision with several frames per launch: NOT configs[1] (whose batch is 1)
        oc = []
        for b_, s_ in ((2, 4), (4, 3), (28, 3)):
            r_, gf_, _ = served_leg(ys, ks, local, b_, streams[:s_], a.precision, max(30, min(a.steps, 100)), kp3d, cam_K,
                                    "not configs[1]: %d frames per launch x %d streams (--detbatch %d)" % (b_, s_, b_) if b_ < 28 else
                                    "not configs[1]: the fp32-accurate arithmetic of the headline at configs[2]'s shape, 28 frames per launch x %d streams "
                                    "(the per-GPU rate of a streamed split, configs[3], at reference-exact parity)" % s_)
            r_["roofline_frac"] = round(gf_ * r_["value"] / 1e3 / {"f32": PEAK_FP32_MFMA_TFLOPS, "bf16x3": PEAK_BF16X3_TFLOPS}.get(a.precision, PEAK_F16_MFMA_TFLOPS), 4)
            oc.append(r_)
        out["other_configs"] = oc
    if a.full and rank == 0 and world == 1 and not a.no_flip_rate:
        # low-margin flip rate of the arg-max stages per arithmetic (betapose_amd/fliprate.py; asserted in tests/test_gpu_flip_rate.py)
        from betapose_amd import fliprate
        out["flip_rate"] = fliprate.measure(device="cuda:%d" % local, trials=2)
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(a.cpu_seconds, kp3d, cam_K)
    if rank == 0:
        print(json.dumps(out), flush=True)
    bpd.finalize()


if __name__ == "__main__":
    main()
