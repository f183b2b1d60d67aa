#!/usr/bin/env python3
"""Time the wideband synthesizer (ofdmrx_util_synthesize, k_synthesize.hip) on resident rows.

At D = 6 and D = 24, with hipEvents on the handle's stream, median of `--reps` after `--warmup`:
  1, 16 and 256 channels that overlap fully (every channel meets every tile), each of `--samples` / D sample frames, and
  256 channels laid end to end (the Monte-Carlo case: every tile meets one or two channels and skips the rest), each of
  `--samples` / (16 D) sample frames;
  ms, input + output GB/s, real multiply-adds of the tap sums per second,
  beside k_awgn_tile on a buffer of the output's bytes and beside the arithmetic floor C_met n_out 25 x 2 FMAs at DESIGN.md section
  6's 0.86 ns per wave64 FMA and SIMD (1024 SIMDs) - C_met the channels a tile meets - and which of the two is nearer.
--ratio P/Q times the ratio synthesizer (ofdmrx_util_synthesize_ratio, k_resynthesize.hip; section 4.18) in place of those two, and
beside it k_synthesize at the neighbouring integer D = round(P / Q) on the same input bytes, against the same yardsticks.
--grid times the grid synthesizer (ofdmrx_util_synthesize_grid, k_synthesize_grid.hip; section 4.20) in place of those: D = 2, 8 and
32 with all 2 D slots, D = 32 with 4 and 16 slots, D = 64, 128 and 512 with all slots, overlapping rows of `--samples` outputs
(default 2^22 there), against the same yardsticks - the traffic is the rows, V written and read twice over (16 + 32 bytes per
output) and the output - and, for D <= 32, beside k_synthesize on the same centres, starts and gains in the same run.
--grid P/Q [SLOTS] times the grid synthesizer at a ratio (ofdmrx_util_synthesize_grid_ratio, k_synthesize_grid_ratio.hip; section
4.23): SLOTS rows (a count, or `all`; without it one row and all of them), overlapping rows of `--samples` outputs, in the same run
beside three yardsticks on the same rows: k_awgn_tile on the output's bytes; ofdmrx_util_synthesize_ratio on the same centres, starts
and gains where P / Q <= 32; ofdmrx_util_synthesize_grid at the next power of two >= P where Q = 1 (the same rows in the same slots:
its capture is longer, so the table gives ns per output too).  The traffic counted with V is the rows, V written and read twice over
(8 x 2 Q x 3 bytes per output) and the output.
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
    import numpy as np
    import torch
    import modem_amd

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    rx = modem_amd.Receiver(device=0, stream=stream.cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

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

    rows = []
    interps = (6, 24)
    if args.ratio is not None:
        p, q = (int(v) for v in args.ratio.split("/"))
        interps = ((p, q), min(32, max(2, int(round(p / q)))))
    size_by = interps[0][0] / interps[0][1] if args.ratio is not None else None   # both take the ratio's input rows
    for D in interps:
        for N, layout in ((1, "overlapping"), (16, "overlapping"), (256, "overlapping"), (256, "end to end")):
            Dr = D[0] / D[1] if isinstance(D, tuple) else float(D)
            Ds = Dr if size_by is None else size_by
            n_in = int(args.samples / Ds) if layout == "overlapping" else int(args.samples / (16 * Ds))
            reach = modem_amd.synthesize_support(n_in, D)
            step = 0 if layout == "overlapping" else reach
            starts = np.arange(N, dtype=np.int64) * step + np.arange(N) % (D[0] if isinstance(D, tuple) else D)
            n_out = int(starts[-1]) + reach
            f = np.linspace(-0.45, 0.45, N) * Dr * 8000.0 + 0.123
            g = np.full(N, 0.5 / (N if layout == "overlapping" else 1), np.float32)
            d_in = torch.randint(-20000, 20000, (N, n_in, 2), dtype=torch.int16, device=dev, generator=gen)
            d_out = torch.empty((n_out, 2), dtype=torch.int16, device=dev)
            ms = timed(lambda k: rx.synthesize(d_in.data_ptr(), 0, n_in, D, f, starts, g, 0, n_out, d_out.data_ptr(), 0))
            spf = 4096
            frames = max(1, n_out // spf)
            d_a = torch.zeros((frames, spf, 2), dtype=torch.int16, device=dev)
            d_b = torch.empty_like(d_a)
            awgn = timed(lambda k: rx.awgn_tile(d_a.data_ptr(), frames, d_b.data_ptr(), frames, spf, -30.0, 7, k * frames))
            met = N if layout == "overlapping" else 1
            floor = met * n_out * 25 * 2 / 64.0 * FMA_NS * 1e-6 / SIMDS
            nbytes = N * n_in * 4 + n_out * 4
            rows.append(dict(interp="%d/%d" % D if isinstance(D, tuple) else D, channels=N, layout=layout, n_out=n_out, ms=round(ms, 4), gb_per_s=round(nbytes / ms / 1e6, 1),
                             gmac_per_s=round(met * n_out * 50 / ms / 1e6, 1), awgn_tile_ms=round(awgn, 4), fma_floor_ms=round(floor, 4),
                             nearer="arithmetic" if floor > awgn else "memory", over_bound=round(ms / max(floor, awgn), 2)))
            del d_in, d_out, d_a, d_b
    rx.close()
    print("interp channels layout        n_out      ms    GB/s  GMAC/s  awgn_tile ms  FMA floor ms  nearer bound  time / bound")
    for r in rows:
        print("%6s %8d %-12s %8d %8.4f %7.1f %7.1f %13.4f %13.4f  %-12s %6.2f" % (
            r["interp"], r["channels"], r["layout"], r["n_out"], r["ms"], r["gb_per_s"], r["gmac_per_s"], r["awgn_tile_ms"], r["fma_floor_ms"],
            r["nearer"], r["over_bound"]))
    print(json.dumps({"tool": "synthesize_bench", "samples": args.samples, "rows": rows}), flush=True)


def child_grid(args):
    import numpy as np
    import torch
    import modem_amd

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    rx = modem_amd.Receiver(device=0, stream=stream.cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

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

    rows = []
    for D, N in ((2, 4), (8, 16), (32, 64), (32, 4), (32, 16), (64, 128), (128, 256), (512, 1024)):
        n_in = args.samples // D
        slots = np.arange(-D, D, dtype=np.int32) if N == 2 * D else (np.arange(N, dtype=np.int32) * (2 * D // N) - D)
        starts = (np.arange(N, dtype=np.int64) % 5) * D
        n_out = int(starts.max()) + modem_amd.synthesize_support(n_in, D)
        g = np.full(N, 0.5 / N, np.float32)
        d_in = torch.randint(-20000, 20000, (N, n_in, 2), dtype=torch.int16, device=dev, generator=gen)
        d_out = torch.empty((n_out, 2), dtype=torch.int16, device=dev)
        ms = timed(lambda k: rx.synthesize_grid(d_in.data_ptr(), 0, n_in, D, slots, starts, g, 0, n_out, d_out.data_ptr(), 0))
        plain = None
        if D <= 32:
            f = modem_amd.grid_centres(D, 8000, slots)
            plain = timed(lambda k: rx.synthesize(d_in.data_ptr(), 0, n_in, D, f, starts, g, 0, n_out, d_out.data_ptr(), 0))
        spf = 4096
        frames = max(1, n_out // spf)
        d_a = torch.zeros((frames, spf, 2), dtype=torch.int16, device=dev)
        d_b = torch.empty_like(d_a)
        awgn = timed(lambda k: rx.awgn_tile(d_a.data_ptr(), frames, d_b.data_ptr(), frames, spf, -30.0, 7, k * frames))
        # arithmetic: the output's 25 x 2 FMAs, and per input time M / 2 log2 M butterflies of 10 operations (6 of them FMA-like issues)
        logm = (2 * D).bit_length() - 1
        floor = (n_out * 25 * 2 + (n_out / D) * D * logm * 6) / 64.0 * FMA_NS * 1e-6 / SIMDS
        nbytes = N * n_in * 4 + n_out * 4
        traffic = nbytes + n_out * 48
        rows.append(dict(interp=D, slots=N, n_out=n_out, ms=round(ms, 4), gb_per_s=round(nbytes / ms / 1e6, 1), traffic_gb_per_s=round(traffic / ms / 1e6, 1),
                         awgn_tile_ms=round(awgn, 4), fma_floor_ms=round(floor, 4), nearer="arithmetic" if floor > awgn else "memory",
                         over_bound=round(ms / max(floor, awgn), 2), k_synthesize_ms=None if plain is None else round(plain, 4),
                         ratio=None if plain is None else round(plain / ms, 2)))
        del d_in, d_out, d_a, d_b
    chunk = {D: modem_amd.synthesize_grid_chunk(D) for D in (2, 8, 32, 64, 128, 512)}
    rx.close()
    print("interp slots    n_out      ms  in+out GB/s  with V GB/s  awgn_tile ms  FMA floor ms  nearer bound  time / bound  k_synthesize ms  k_synthesize / grid")
    for r in rows:
        print("%6d %5d %8d %7.4f %12.1f %12.1f %13.4f %13.4f  %-12s %6.2f %16s %10s" % (
            r["interp"], r["slots"], r["n_out"], r["ms"], r["gb_per_s"], r["traffic_gb_per_s"], r["awgn_tile_ms"], r["fma_floor_ms"], r["nearer"],
            r["over_bound"], "-" if r["k_synthesize_ms"] is None else "%.4f" % r["k_synthesize_ms"], "-" if r["ratio"] is None else "%.2f" % r["ratio"]))
    print(json.dumps({"tool": "synthesize_bench", "grid": True, "samples": args.samples, "chunk_outputs": chunk, "rows": rows}), flush=True)


def child_grid_ratio(args):
    import numpy as np
    import torch
    import modem_amd

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    rx = modem_amd.Receiver(device=0, stream=stream.cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

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

    p, q = (int(v) for v in args.grid[0].split("/"))
    g0 = math.gcd(p, q)
    p, q = p // g0, q // g0
    every = modem_amd.grid_centres((p, q), 8000).size
    counts = [1, every] if len(args.grid) < 2 else [every if args.grid[1] == "all" else int(args.grid[1])]
    k_first = -(p // q)
    rows = []
    for N in counts:
        n_in = args.samples * q // p
        slots = (np.arange(N, dtype=np.int32) * (every // N) + k_first).astype(np.int32)
        starts = (np.arange(N, dtype=np.int64) % 5) * p
        n_out = int(starts.max()) + modem_amd.synthesize_support(n_in, (p, q))
        g = np.full(N, 0.5 / N, np.float32)
        d_in = torch.randint(-20000, 20000, (N, n_in, 2), dtype=torch.int16, device=dev, generator=gen)
        d_out = torch.empty((n_out, 2), dtype=torch.int16, device=dev)
        ms = timed(lambda k: rx.synthesize_grid(d_in.data_ptr(), 0, n_in, (p, q), slots, starts, g, 0, n_out, d_out.data_ptr(), 0))
        direct = None
        if p <= 32 * q:
            f = modem_amd.grid_centres((p, q), 8000, slots)
            direct = timed(lambda k: rx.synthesize(d_in.data_ptr(), 0, n_in, (p, q), f, starts, g, 0, n_out, d_out.data_ptr(), 0))
        pow2, pow2_out = None, None
        if q == 1:
            D = 1 << (p - 1).bit_length()
            s2 = (np.arange(N, dtype=np.int64) % 5) * D
            pow2_out = int(s2.max()) + modem_amd.synthesize_support(n_in, D)
            d_o2 = torch.empty((pow2_out, 2), dtype=torch.int16, device=dev)
            pow2 = timed(lambda k: rx.synthesize_grid(d_in.data_ptr(), 0, n_in, D, slots, s2, g, 0, pow2_out, d_o2.data_ptr(), 0))
            del d_o2
        spf = 4096
        frames = max(1, n_out // spf)
        d_a = torch.zeros((frames, spf, 2), dtype=torch.int16, device=dev)
        d_b = torch.empty_like(d_a)
        awgn = timed(lambda k: rx.awgn_tile(d_a.data_ptr(), frames, d_b.data_ptr(), frames, spf, -30.0, 7, k * frames))
        nbytes = N * n_in * 4 + n_out * 4
        traffic = nbytes + n_out * 8 * 2 * q * 3
        rows.append(dict(ratio="%d/%d" % (p, q), slots=N, n_out=n_out, ms=round(ms, 4), ns_per_output=round(ms * 1e6 / n_out, 4),
                         gb_per_s=round(nbytes / ms / 1e6, 1), traffic_gb_per_s=round(traffic / ms / 1e6, 1), awgn_tile_ms=round(awgn, 4),
                         over_awgn=round(ms / awgn, 2), synthesize_ratio_ms=None if direct is None else round(direct, 4),
                         synthesize_ratio_over_grid=None if direct is None else round(direct / ms, 2),
                         synthesize_grid_pow2_ms=None if pow2 is None else round(pow2, 4),
                         synthesize_grid_pow2_ns_per_output=None if pow2 is None else round(pow2 * 1e6 / pow2_out, 4)))
        del d_in, d_out, d_a, d_b
    chunk = modem_amd.synthesize_grid_chunk((p, q))
    rx.close()
    print(" ratio slots    n_out       ms  ns/output  in+out GB/s  with V GB/s  awgn_tile ms  time / awgn  synthesize_ratio ms  ratio / grid  grid at 2^n ms  its ns/output")
    dash = lambda v, fmt: "-" if v is None else fmt % v
    for r in rows:
        print("%6s %5d %8d %8.4f %10.4f %12.1f %12.1f %13.4f %12.2f %20s %13s %15s %14s" % (
            r["ratio"], r["slots"], r["n_out"], r["ms"], r["ns_per_output"], r["gb_per_s"], r["traffic_gb_per_s"], r["awgn_tile_ms"], r["over_awgn"],
            dash(r["synthesize_ratio_ms"], "%.4f"), dash(r["synthesize_ratio_over_grid"], "%.2f"), dash(r["synthesize_grid_pow2_ms"], "%.4f"),
            dash(r["synthesize_grid_pow2_ns_per_output"], "%.4f")))
    print(json.dumps({"tool": "synthesize_bench", "grid": "%d/%d" % (p, q), "samples": args.samples, "chunk_outputs": chunk, "rows": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=None, help="wideband samples an overlapping channel spans (2^20; --grid: 2^22)")
    ap.add_argument("--grid", nargs="*", default=None, metavar="ARG",
                    help="alone: the grid synthesizer, beside k_synthesize for D <= 32; P/Q [SLOTS]: the grid synthesizer at a ratio beside its yardsticks")
    ap.add_argument("--ratio", default=None, help="P/Q: the ratio synthesizer beside k_synthesize at round(P / Q)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds the GPU step may take")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.samples is None:
        args.samples = 1 << 22 if args.grid is not None else 1 << 20
    if args.grid and ("/" not in args.grid[0] or len(args.grid) > 2):
        ap.error("--grid takes nothing, or P/Q and an optional count of slots (or `all`)")
    if args.child:
        return child_grid_ratio(args) if args.grid else child_grid(args) if args.grid is not None else child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--samples", str(args.samples), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    if args.ratio is not None:
        cmd += ["--ratio", args.ratio]
    if args.grid is not None:
        cmd += ["--grid"] + args.grid
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print("synthesize_bench: the GPU step ran into its time limit of %d s" % args.timeout, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
