#!/usr/bin/env python3
"""Time the wideband survey (ofdmrx_util_survey, k_survey.hip) on a resident S16 capture.

For every transform length (1280, 2560, 5120), one row over the whole capture and waterfalls of rows of 64 and of 8 segments (8: one
group per row, so the second launch has nothing to add up - the difference to one row is the ordered sum over the groups), with hipEvents
on the handle's stream, median of `--reps` after `--warmup`:
  ms, segments, input GB/s, transforms per second,
  beside k_awgn_tile on a buffer of the same bytes (the comparison DESIGN.md 4.13 / 4.14 used) and beside the arithmetic floor of
  the transforms - per segment 2.5 N log2 N fused multiply-adds (5 N log2 N flops, every pair taken as one FMA) + 2 N products of
  the window + 2 N of |X|^2 - at DESIGN.md section 6's 0.86 ns per wave64 FMA and SIMD (1024 SIMDs), and which of the two is nearer.
`--grid [D ...]` times the grid survey instead (ofdmrx_util_survey_grid, k_survey_grid.hip): for every D
(default 2, 8, 32, 64, 128, 512) the two launches at S = 4096 and at S = 8 output times per row (8: one group per row, so the second
launch has nothing to add up and the row isolates the first kernel) over every whole row of the capture, beside k_channelize_grid
storing ALL slots of the same output times of the same capture in the same run - the same arithmetic, 16 x the bytes written - and
beside k_awgn_tile on the capture's bytes.
`--grid-ratio [P/Q ...]` times the grid survey at a ratio (ofdmrx_util_survey_grid_ratio, k_survey_grid_ratio.hip; DESIGN.md section
4.24): for every ratio (default 6/1, 30/1, 25/4, 125/4, 300/1) the two launches at S = 4096 and at S = 8 over every whole row of the
capture, beside ofdmrx_util_channelize_grid_ratio storing ALL slots of the same output times of the same capture in the same run,
beside k_awgn_tile on the capture's bytes and - for Q = 1 - beside ofdmrx_util_survey_grid at the next power of two over the same
number of rows.
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


def grid_child(args):
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
    for D in args.grid:
        M = 2 * D
        times = ((W - 1) // D + 1) // 4096 * 4096                    # whole rows of 4096: the same output times for every entry
        d_all = torch.empty((M, times, 2), dtype=torch.float32, device=dev)

        def front(k):
            assert L.ofdmrx_util_channelize_grid(h, d_in.data_ptr(), 0, 0, W, D, None, M, 0, times, d_all.data_ptr(), times) == 0

        chg = timed(front)
        for S in (4096, 8):
            n_rows = times // S
            d_out = torch.empty((n_rows, M), dtype=torch.float32, device=dev)

            def run(k):
                assert L.ofdmrx_util_survey_grid(h, d_in.data_ptr(), 0, 0, W, D, S, 0, n_rows, d_out.data_ptr()) == 0

            ms = timed(run)
            rows.append(dict(decim=D, times_per_row=S, rows=n_rows, times=times, ms=round(ms, 4), channelize_grid_ms=round(chg, 4),
                             ratio=round(ms / chg, 3), gb_per_s=round(nbytes / ms / 1e6, 1), awgn_tile_ms=round(awgn, 4)))
            del d_out
        del d_all
    rx.close()
    print("    D  times/row    rows     times  survey ms  channelize_grid ms  survey / front end  input GB/s  awgn_tile ms")
    for r in rows:
        print("%5d %10d %7d %9d %10.4f %19.4f %19.3f %11.1f %13.4f" % (r["decim"], r["times_per_row"], r["rows"], r["times"], r["ms"],
                                                                    r["channelize_grid_ms"], r["ratio"], r["gb_per_s"], r["awgn_tile_ms"]))
    print(json.dumps({"tool": "survey_bench --grid", "samples": W, "rows": rows}), flush=True)


def ratio_child(args):
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
    for text in args.grid_ratio:
        P, Q = (int(v) for v in text.split("/"))
        g = math.gcd(P, Q)
        P, Q = P // g, Q // g
        n_all = len(modem_amd.grid_centres((P, Q), 8000))
        times = ((W * Q - 1) // P + 1) // 4096 * 4096                # whole rows of 4096: the same output times for every entry
        d_all = torch.empty((n_all, times, 2), dtype=torch.float32, device=dev)

        def front(k):
            assert L.ofdmrx_util_channelize_grid_ratio(h, d_in.data_ptr(), 0, 0, W, P, Q, None, n_all, 0, times, d_all.data_ptr(), times) == 0

        chg = timed(front)
        D2 = 1 << (P - 1).bit_length() if Q == 1 and P & (P - 1) else 0   # the next power of two
        for S in (4096, 8):
            n_rows = times // S
            d_out = torch.empty((n_rows, n_all), dtype=torch.float32, device=dev)

            def run(k):
                assert L.ofdmrx_util_survey_grid_ratio(h, d_in.data_ptr(), 0, 0, W, P, Q, S, 0, n_rows, d_out.data_ptr()) == 0

            ms = timed(run)
            pow2 = None
            if D2 and D2 <= 512:
                rows2 = min(n_rows, ((W - 1) // D2 + 1) // S)
                d_out2 = torch.empty((rows2, 2 * D2), dtype=torch.float32, device=dev)

                def run2(k):
                    assert L.ofdmrx_util_survey_grid(h, d_in.data_ptr(), 0, 0, W, D2, S, 0, rows2, d_out2.data_ptr()) == 0

                pow2 = dict(decim=D2, rows=rows2, ms=round(timed(run2), 4))
                del d_out2
            rows.append(dict(ratio="%d/%d" % (P, Q), slots=n_all, times_per_row=S, rows=n_rows, times=times, ms=round(ms, 4),
                             channelize_grid_ratio_ms=round(chg, 4), survey_over_front_end=round(ms / chg, 3),
                             gb_per_s=round(times * P // Q * 4 / ms / 1e6, 1), awgn_tile_ms=round(awgn, 4), survey_grid_pow2=pow2))
            del d_out
        del d_all
    rx.close()
    print("   P/Q  slots  times/row    rows     times  survey ms  channelize_grid_ratio ms  survey / front end  input GB/s  awgn_tile ms  survey_grid at 2^n (rows): ms")
    for r in rows:
        p2 = r["survey_grid_pow2"]
        print("%6s %6d %10d %7d %9d %10.4f %25.4f %19.3f %11.1f %13.4f  %s" % (
            r["ratio"], r["slots"], r["times_per_row"], r["rows"], r["times"], r["ms"], r["channelize_grid_ratio_ms"], r["survey_over_front_end"],
            r["gb_per_s"], r["awgn_tile_ms"], "D %d (%d): %.4f" % (p2["decim"], p2["rows"], p2["ms"]) if p2 else "-"))
    print(json.dumps({"tool": "survey_bench --grid-ratio", "samples": W, "rows": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid-ratio", nargs="*", default=None, help="time the grid survey at these ratios P/Q (none given: 6/1 30/1 25/4 125/4 300/1)")
    ap.add_argument("--grid", type=int, nargs="*", default=None, help="time the grid survey at these decimations (none given: 2 8 32 64 128 512)")
    ap.add_argument("--samples", type=int, default=None, help="default 2^20 (2^22 with --grid or --grid-ratio)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=120, help="seconds the GPU step may take")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.grid is not None and not args.grid:
        args.grid = [2, 8, 32, 64, 128, 512]
    if args.grid_ratio is not None and not args.grid_ratio:
        args.grid_ratio = ["6/1", "30/1", "25/4", "125/4", "300/1"]
    if args.samples is None:
        args.samples = 1 << (20 if args.grid is None and args.grid_ratio is None else 22)
    if args.child:
        if args.grid_ratio is not None:
            return ratio_child(args)
        return child(args) if args.grid is None else grid_child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--samples", str(args.samples), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    if args.grid is not None:
        cmd += ["--grid"] + [str(d) for d in args.grid]
    if args.grid_ratio is not None:
        cmd += ["--grid-ratio"] + list(args.grid_ratio)
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print("survey_bench: the GPU step ran into its time limit of %d s" % args.timeout, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
