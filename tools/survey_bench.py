#!/usr/bin/env python3
"""Time the wideband survey (ofdmrx_util_survey, k_survey.hip) on a resident S16 capture.

For every transform length (1280, 2560, 5120), one row over the whole capture and waterfalls of rows of 64 and of 8 segments (8: one
group per row, so the second launch has nothing to add up - the difference to one row is the ordered sum over the groups), with hipEvents
on the handle's stream, median of `--reps` after `--warmup`:
  ms, segments, input GB/s, transforms per second,
  beside k_awgn_tile on a buffer of the same bytes (the comparison DESIGN.md 4.13 / 4.14 used) and beside the arithmetic floor of
  the transforms - per segment 2.5 N log2 N fused multiply-adds (5 N log2 N flops, every pair taken as one FMA) + 2 N products of
  the window + 2 N of |X|^2 - at DESIGN.md section 6's 0.86 ns per wave64 FMA and SIMD (1024 SIMDs), and which of the two is nearer.
The GPU work runs in a child process under a time limit; the parent never opens the GPU.  Prints a table and one JSON line."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FMA_NS, SIMDS = 0.86, 1024


def child(args):
    import torch
    import modem_amd

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    rx = modem_amd.Receiver(device=0, stream=stream.cuda_stream)
    W = args.samples
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    d_in = torch.randint(-20000, 20000, (W, 2), dtype=torch.int16, device=dev, generator=gen)

    def timed(f):
        ms = []
        for k in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            f(k)
            b.record(stream)
            b.synchronize()
            if k >= args.warmup:
                ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    nbytes = W * 4
    spf = 4096
    frames = max(1, nbytes // (2 * spf * 4))
    d_a = torch.zeros((frames, spf, 2), dtype=torch.int16, device=dev)
    d_b = torch.empty_like(d_a)
    awgn = timed(lambda k: rx.awgn_tile(d_a.data_ptr(), frames, d_b.data_ptr(), frames, spf, -30.0, 7, k * frames))
    rows = []
    L, h = rx._lib, rx._h
    for N in (1280, 2560, 5120):
        total = (W - N // 2) // (N // 2)
        for S in (min(total, 65536), 64, 8):
            n_rows = total // S
            d_out = torch.empty((n_rows, N), dtype=torch.float32, device=dev)

            def run(k):
                assert L.ofdmrx_util_survey(h, d_in.data_ptr(), 0, 0, W, N, S, 0, n_rows, d_out.data_ptr()) == 0

            ms = timed(run)
            segs = n_rows * S
            floor = segs * (2.5 * N * math.log2(N) + 4 * N) / 64.0 * FMA_NS * 1e-6 / SIMDS
            rows.append(dict(nfft=N, segs_per_row=S, rows=n_rows, segments=segs, workgroups=n_rows * -(-S // 8), ms=round(ms, 4),
                             gb_per_s=round(nbytes / ms / 1e6, 1), ktransforms_per_s=round(segs / ms, 1), awgn_tile_ms=round(awgn, 4),
                             fma_floor_ms=round(floor, 5), nearer="arithmetic" if floor > awgn else "memory", over_bound=round(ms / max(floor, awgn), 2)))
            del d_out
    rx.close()
    print(" nfft  segs/row  rows  workgroups      ms    GB/s  ktransf/s  awgn_tile ms  FMA floor ms  nearer bound  time / bound")
    for r in rows:
        print("%5d %9d %5d %11d %7.4f %7.1f %10.1f %13.4f %13.5f  %-12s %6.2f" % (r["nfft"], r["segs_per_row"], r["rows"], r["workgroups"], r["ms"],
                                                                                r["gb_per_s"], r["ktransforms_per_s"], r["awgn_tile_ms"],
                                                                                r["fma_floor_ms"], r["nearer"], r["over_bound"]))
    print(json.dumps({"tool": "survey_bench", "samples": W, "rows": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=120, help="seconds the GPU step may take")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--samples", str(args.samples), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print("survey_bench: the GPU step ran into its time limit of %d s" % args.timeout, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
