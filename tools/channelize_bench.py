#!/usr/bin/env python3
"""Time the wideband front end (ofdmrx_util_channelize, k_channelize.hip) on a resident capture.

For 1, 16 and 256 channels at D = 6 and D = 24, with hipEvents on the handle's stream, median of `--reps` after `--warmup`:
  ms, input + output GB/s, complex multiply-adds per second,
  beside k_awgn_tile on a buffer of the same bytes (the comparison DESIGN.md 4.13 used) and beside the arithmetic floor
  N n_out T 4 FMAs at DESIGN.md section 6's 0.86 ns per wave64 FMA and SIMD (1024 SIMDs), and which of the two is nearer.
Then one wideband-bank push of one second x 64 channels against ofdmrx_util_channelize + copy to host + ofdmrx_bank_push of the same
data (host wall time: these calls block).
--ratio P/Q (repeatable) times the front end at a rational decimation instead (ofdmrx_util_channelize_ratio, k_rechannelize;
DESIGN.md section 4.17): for 1, 16 and 256 channels, beside k_channelize at the neighbouring integer D on the same bytes, beside
k_awgn_tile and the arithmetic floor N n_out T 4 FMAs, with the time per FMA relative to k_channelize's; then one wideband second x
64 channels through the ratio bank.
--grid D [SLOTS] (repeatable; SLOTS a comma list, default all 2 D; D:SLOTS where the list begins with a negative slot) times the grid front end instead (ofdmrx_util_channelize_grid,
k_channelize_grid.hip) beside three yardsticks: k_awgn_tile on the same bytes; the arithmetic floor - per
output time 13 M real-by-complex multiply-adds (2 FMAs each) and (M / 2) log2 M butterflies of 8 operations - at the same 0.86 ns per
wave64 FMA and SIMD; and, for D <= 32, k_channelize on the same centres in the same run.  Then one wideband second through the grid
bank with those slots.
--grid P/Q [SLOTS] (repeatable; the spelling with `/`) times the grid front end at a ratio (ofdmrx_util_channelize_grid_ratio,
k_channelize_grid_ratio.hip), with one slot (slot 0, or SLOTS) and with all slots, beside: the direct form
(k_rechannelize / k_channelize) on the same centres in the same run where P / Q <= 32; k_channelize_grid at the next power of two
>= P on the same samples, for Q = 1; k_awgn_tile on the same bytes.
--real [P/Q] (repeatable; no value: D = 6, 16 and 32; a bare integer is that D) times the front end for a REAL capture
(ofdmrx_util_channelize_real, k_channelize.hip) beside the analytic front end on the same number of
wideband samples and the same centres in the same run, for 4 and 64 channels (--channels): each figure is the time of one launch
from events round --inner launches, the median of --reps such groups with the least and the most beside it.
The GPU work runs in a child process under a time limit; the parent never opens the GPU.  Prints a table and one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FMA_NS, SIMDS = 0.86, 1024


def child(args):
    import numpy as np
    import torch
    import modem_amd
    import modem_amd.ofdmrx as M

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

    rows = []
    for D in (6, 24):
        T = 24 * D + 1
        n_out = -(-W // D)
        for N in (1, 16, 256):
            f = np.linspace(-0.45, 0.45, N) * D * 8000.0 + 0.123
            d_out = torch.empty((N, n_out, 2), dtype=torch.float32, device=dev)
            ms = timed(lambda k: rx.channelize(d_in.data_ptr(), 0, 0, W, D, f, 0, n_out, d_out.data_ptr()))
            nbytes = W * 4 + N * n_out * 8
            spf = 4096
            frames = max(1, nbytes // (2 * spf * 4))
            d_a = torch.zeros((frames, spf, 2), dtype=torch.int16, device=dev)
            d_b = torch.empty_like(d_a)
            awgn = timed(lambda k: rx.awgn_tile(d_a.data_ptr(), frames, d_b.data_ptr(), frames, spf, -30.0, 7, k * frames))
            floor = N * n_out * T * 4 / 64.0 * FMA_NS * 1e-6 / SIMDS
            rows.append(dict(decim=D, channels=N, ms=round(ms, 4), gb_per_s=round(nbytes / ms / 1e6, 1), gmac_per_s=round(N * n_out * T / ms / 1e6, 1),
                             awgn_tile_ms=round(awgn, 4), fma_floor_ms=round(floor, 4), nearer="arithmetic" if floor > awgn else "memory",
                             over_bound=round(ms / max(floor, awgn), 2)))
            del d_out, d_a, d_b
    rx.close()

    # one second x 64 channels through the wideband bank, and through channelize + copy + a plain bank
    D, N, sec = 6, 64, 48000
    f = np.linspace(-0.45, 0.45, N) * D * 8000.0 + 0.123
    rng = np.random.default_rng(2)
    cap = rng.integers(-300, 300, size=((args.warmup + args.reps) * sec, 2)).astype(np.int16)
    outs = (np.zeros((64, 5380), np.uint8), np.zeros(64, M.RESULT_DTYPE), np.zeros(64, np.int32), np.zeros(64, np.int64))
    a, b = C.c_size_t(0), C.c_size_t(0)
    p = M._ptr
    rxw = modem_amd.Receiver(device=0)
    L, h = rxw._lib, rxw._h
    assert L.ofdmrx_bank_begin_wideband(h, N, p(f), D, 0) == 0
    wide = []
    for k in range(args.warmup + args.reps):
        blk = np.ascontiguousarray(cap[k * sec:(k + 1) * sec])
        t = time.perf_counter()
        assert L.ofdmrx_bank_push_wideband(h, p(blk), sec, 0, 64, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), C.byref(a), C.byref(b)) == 0
        wide.append((time.perf_counter() - t) * 1e3)
    wide_ops = int(L.ofdmrx_bank_last_stage_ops(h))
    rxw.close()
    rxc, rxb = modem_amd.Receiver(device=0), modem_amd.Receiver(device=0)
    d_cap = torch.from_numpy(cap).to(dev)
    n_blk = sec // D
    d_rows = torch.empty((N, n_blk, 2), dtype=torch.float32, device=dev)
    host = torch.empty((N, n_blk, 2), dtype=torch.float32).pin_memory()
    torch.cuda.synchronize()
    assert rxb._lib.ofdmrx_bank_begin(rxb._h, N, 2, 2) == 0
    lens = np.full(N, n_blk, np.uintp)
    plain = []
    for k in range(args.warmup + args.reps):
        i0 = max(0, k * sec - 24 * D)
        t = time.perf_counter()
        rxc.channelize(d_cap.data_ptr() + 4 * i0, 0, i0, (k + 1) * sec - i0, D, f, k * n_blk, n_blk, d_rows.data_ptr())
        rxc.synchronize()
        host.copy_(d_rows)
        assert rxb._lib.ofdmrx_bank_push(rxb._h, host.data_ptr(), n_blk * 8, p(lens), None, 64, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]),
                                         C.byref(a), C.byref(b)) == 0
        plain.append((time.perf_counter() - t) * 1e3)
    plain_ops = int(rxb._lib.ofdmrx_bank_last_stage_ops(rxb._h))
    rxc.close()
    rxb.close()
    w = args.warmup
    bank = dict(channels=N, decim=D, wideband_push_ms=round(statistics.median(wide[w:]), 3), wideband_stage_ops=wide_ops,
                channelize_copy_push_ms=round(statistics.median(plain[w:]), 3), plain_stage_ops=plain_ops)
    print("decim channels      ms    GB/s  GMAC/s  awgn_tile ms  FMA floor ms  nearer bound  time / bound")
    for r in rows:
        print("%5d %8d %7.4f %7.1f %7.1f %13.4f %13.4f  %-12s %6.2f" % (r["decim"], r["channels"], r["ms"], r["gb_per_s"], r["gmac_per_s"],
                                                                      r["awgn_tile_ms"], r["fma_floor_ms"], r["nearer"], r["over_bound"]))
    print("one wideband second x %d channels: wideband bank push %.3f ms (%d stage ops); channelize + copy + plain bank push %.3f ms (%d stage ops)"
          % (N, bank["wideband_push_ms"], wide_ops, bank["channelize_copy_push_ms"], plain_ops))
    print(json.dumps({"tool": "channelize_bench", "samples": W, "rows": rows, "bank": bank}), flush=True)


def child_ratio(args):
    import numpy as np
    import torch
    import modem_amd
    import modem_amd.ofdmrx as M

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

    ratios = [tuple(int(t) for t in r.split("/")) for r in args.ratio]
    rows = []
    for P, Q in ratios:
        T = 24 * P // Q + 1
        n_out = -(-W * Q // P)
        D = min(32, max(2, int(round(P / Q))))                        # the neighbouring integer decimation, on the same bytes
        Ti, ni = 24 * D + 1, -(-W // D)
        for N in (1, 16, 256):
            f = np.linspace(-0.45, 0.45, N) * 8000.0 * P / Q + 0.123
            d_out = torch.empty((N, max(n_out, ni), 2), dtype=torch.float32, device=dev)
            ms = timed(lambda k: rx.channelize(d_in.data_ptr(), 0, 0, W, (P, Q), f, 0, n_out, d_out.data_ptr()))
            fi = np.linspace(-0.45, 0.45, N) * 8000.0 * D + 0.123
            msi = timed(lambda k: rx.channelize(d_in.data_ptr(), 0, 0, W, D, fi, 0, ni, d_out.data_ptr()))
            nbytes = W * 4 + N * n_out * 8
            spf = 4096
            frames = max(1, nbytes // (2 * spf * 4))
            d_a = torch.zeros((frames, spf, 2), dtype=torch.int16, device=dev)
            d_b = torch.empty_like(d_a)
            awgn = timed(lambda k: rx.awgn_tile(d_a.data_ptr(), frames, d_b.data_ptr(), frames, spf, -30.0, 7, k * frames))
            floor = N * n_out * T * 4 / 64.0 * FMA_NS * 1e-6 / SIMDS
            per_fma = (ms / (N * n_out * T)) / (msi / (N * ni * Ti))
            rows.append(dict(ratio="%d/%d" % (P, Q), taps=T, channels=N, ms=round(ms, 4), gb_per_s=round(nbytes / ms / 1e6, 1),
                             gmac_per_s=round(N * n_out * T / ms / 1e6, 1), integer_decim=D, k_channelize_ms=round(msi, 4),
                             time_per_fma_vs_k_channelize=round(per_fma, 2), awgn_tile_ms=round(awgn, 4), fma_floor_ms=round(floor, 4),
                             nearer="arithmetic" if floor > awgn else "memory", over_bound=round(ms / max(floor, awgn), 2)))
            del d_out, d_a, d_b
    rx.close()

    # one wideband second x 64 channels through the ratio bank
    N = 64
    outs = (np.zeros((64, 5380), np.uint8), np.zeros(64, M.RESULT_DTYPE), np.zeros(64, np.int32), np.zeros(64, np.int64))
    a, b = C.c_size_t(0), C.c_size_t(0)
    p = M._ptr
    banks = []
    for P, Q in ratios:
        if 8000 * P % Q:
            continue
        sec = 8000 * P // Q
        f = np.linspace(-0.45, 0.45, N) * sec + 0.123
        rng = np.random.default_rng(2)
        cap = rng.integers(-300, 300, size=((args.warmup + args.reps) * sec, 2)).astype(np.int16)
        rxw = modem_amd.Receiver(device=0)
        L, h = rxw._lib, rxw._h
        assert L.ofdmrx_bank_begin_wideband_ratio(h, N, p(f), P, Q, 0) == 0
        wide = []
        for k in range(args.warmup + args.reps):
            blk = np.ascontiguousarray(cap[k * sec:(k + 1) * sec])
            t = time.perf_counter()
            assert L.ofdmrx_bank_push_wideband(h, p(blk), sec, 0, 64, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), C.byref(a), C.byref(b)) == 0
            wide.append((time.perf_counter() - t) * 1e3)
        ops = int(L.ofdmrx_bank_last_stage_ops(h))
        rxw.close()
        banks.append(dict(ratio="%d/%d" % (P, Q), channels=N, wideband_samples=sec, push_ms=round(statistics.median(wide[args.warmup:]), 3), stage_ops=ops))
    print("ratio     T channels      ms    GB/s  GMAC/s  k_channelize D ms  t/FMA vs it  awgn_tile ms  FMA floor ms  nearer bound  time / bound")
    for r in rows:
        print("%-7s %3d %8d %7.4f %7.1f %7.1f %9d %9.4f %10.2f %13.4f %13.4f  %-12s %6.2f"
              % (r["ratio"], r["taps"], r["channels"], r["ms"], r["gb_per_s"], r["gmac_per_s"], r["integer_decim"], r["k_channelize_ms"],
                 r["time_per_fma_vs_k_channelize"], r["awgn_tile_ms"], r["fma_floor_ms"], r["nearer"], r["over_bound"]))
    for k in banks:
        print("one wideband second (%d samples at %s) x %d channels through the ratio bank: push %.3f ms (%d stage ops)"
              % (k["wideband_samples"], k["ratio"], k["channels"], k["push_ms"], k["stage_ops"]))
    print(json.dumps({"tool": "channelize_bench", "samples": W, "ratio_rows": rows, "ratio_banks": banks}), flush=True)


def child_grid(args):
    import numpy as np
    import torch
    import modem_amd
    import modem_amd.ofdmrx as M

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

    grids = []
    for g in args.grid:                                               # D, D SLOTS or D:SLOTS (a list that begins with a negative slot)
        g = g[0].split(":") if ":" in g[0] else g
        grids.append((int(g[0]), None if len(g) < 2 else [int(t) for t in g[1].split(",")]))
    rows = []
    for D, slots in grids:
        Mm = 2 * D
        N = Mm if slots is None else len(slots)
        n_out = -(-W // D)
        d_out = torch.empty((N, n_out, 2), dtype=torch.float32, device=dev)
        ms = timed(lambda k: rx.channelize_grid(d_in.data_ptr(), 0, 0, W, D, slots, 0, n_out, d_out.data_ptr()))
        plain = None
        if D <= 32:                                                  # the direct form on the same centres, in the same run
            f = modem_amd.grid_centres(D, 8000, slots)
            plain = timed(lambda k: rx.channelize(d_in.data_ptr(), 0, 0, W, D, f, 0, n_out, d_out.data_ptr()))
        nbytes = W * 4 + N * n_out * 8
        spf = 4096
        frames = max(1, nbytes // (2 * spf * 4))
        d_a = torch.zeros((frames, spf, 2), dtype=torch.int16, device=dev)
        d_b = torch.empty_like(d_a)
        awgn = timed(lambda k: rx.awgn_tile(d_a.data_ptr(), frames, d_b.data_ptr(), frames, spf, -30.0, 7, k * frames))
        ops = n_out * (13 * Mm * 2 + (Mm // 2) * (Mm.bit_length() - 1) * 8)
        floor = ops / 64.0 * FMA_NS * 1e-6 / SIMDS
        rows.append(dict(decim=D, slots=N, n_out=n_out, ms=round(ms, 4), gb_per_s=round(nbytes / ms / 1e6, 1),
                         k_channelize_ms=None if plain is None else round(plain, 4), speedup=None if plain is None else round(plain / ms, 2),
                         awgn_tile_ms=round(awgn, 4), floor_ms=round(floor, 4), nearer="arithmetic" if floor > awgn else "memory",
                         over_bound=round(ms / max(floor, awgn), 2)))
        del d_out, d_a, d_b
    rx.close()

    outs = (np.zeros((64, 5380), np.uint8), np.zeros(64, M.RESULT_DTYPE), np.zeros(64, np.int32), np.zeros(64, np.int64))
    a, b = C.c_size_t(0), C.c_size_t(0)
    p = M._ptr
    banks = []
    for D, slots in grids:
        sec = 8000 * D
        rng = np.random.default_rng(2)
        cap = rng.integers(-300, 300, size=(sec, 2)).astype(np.int16)
        rxw = modem_amd.Receiver(device=0)
        L, h = rxw._lib, rxw._h
        k = M._grid_slots(D, slots)
        assert L.ofdmrx_bank_begin_wideband_grid(h, k.size, p(k), D, 0) == 0
        wide = []
        for _ in range(args.warmup + args.reps):
            t = time.perf_counter()
            assert L.ofdmrx_bank_push_wideband(h, p(cap), sec, 0, 64, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), C.byref(a), C.byref(b)) == 0
            wide.append((time.perf_counter() - t) * 1e3)
        ops = int(L.ofdmrx_bank_last_stage_ops(h))
        rxw.close()
        banks.append(dict(decim=D, slots=int(k.size), wideband_samples=sec, push_ms=round(statistics.median(wide[args.warmup:]), 3), stage_ops=ops))
    print("decim slots   n_out      ms    GB/s  k_channelize ms  speedup  awgn_tile ms  floor ms  nearer bound  time / bound")
    for r in rows:
        print("%5d %5d %7d %7.4f %7.1f %16s %8s %13.4f %9.4f  %-12s %6.2f"
              % (r["decim"], r["slots"], r["n_out"], r["ms"], r["gb_per_s"], "-" if r["k_channelize_ms"] is None else "%.4f" % r["k_channelize_ms"],
                 "-" if r["speedup"] is None else "%.2f" % r["speedup"], r["awgn_tile_ms"], r["floor_ms"], r["nearer"], r["over_bound"]))
    for k in banks:
        print("one wideband second (%d samples, D = %d) x %d slots through the grid bank: push %.3f ms (%d stage ops)"
              % (k["wideband_samples"], k["decim"], k["slots"], k["push_ms"], k["stage_ops"]))
    print(json.dumps({"tool": "channelize_bench", "samples": W, "grid_rows": rows, "grid_banks": banks}), flush=True)


def child_grid_ratio(args):
    import numpy as np
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

    rows = []
    for g in args.grid:
        P, Q = (int(t) for t in g[0].split("/"))
        one = [0] if len(g) < 2 else [int(t) for t in g[1].split(",")]
        n_out = -(-W * Q // P)
        n_all = len(modem_amd.grid_centres((P, Q), 8000))
        pow2 = None
        if Q == 1:                                                   # 4.19's kernel at the next power of two, all its slots, on the same samples
            D2 = 1 << (P - 1).bit_length()
            n2 = -(-W // D2)
            d2 = torch.empty((2 * D2, n2, 2), dtype=torch.float32, device=dev)
            pow2 = (D2, timed(lambda k: rx.channelize_grid(d_in.data_ptr(), 0, 0, W, D2, None, 0, n2, d2.data_ptr())))
            del d2
        for slots in (one, None):
            N = n_all if slots is None else len(slots)
            d_out = torch.empty((N, n_out, 2), dtype=torch.float32, device=dev)
            ms = timed(lambda k: rx.channelize_grid(d_in.data_ptr(), 0, 0, W, (P, Q), slots, 0, n_out, d_out.data_ptr()))
            plain = None
            if P <= 32 * Q:                                          # the direct form on the same centres, in the same run
                f = modem_amd.grid_centres((P, Q), 8000, slots)
                plain = timed(lambda k: rx.channelize(d_in.data_ptr(), 0, 0, W, P if Q == 1 else (P, Q), f, 0, n_out, d_out.data_ptr()))
            nbytes = W * 4 + N * n_out * 8
            spf = 4096
            frames = max(1, nbytes // (2 * spf * 4))
            d_a = torch.zeros((frames, spf, 2), dtype=torch.int16, device=dev)
            d_b = torch.empty_like(d_a)
            awgn = timed(lambda k: rx.awgn_tile(d_a.data_ptr(), frames, d_b.data_ptr(), frames, spf, -30.0, 7, k * frames))
            rows.append(dict(ratio="%d/%d" % (P, Q), m=2 * P, slots=N, n_out=n_out, ms=round(ms, 4), gb_per_s=round(nbytes / ms / 1e6, 1),
                             us_per_slot=round(1e3 * ms / N, 3), direct_ms=None if plain is None else round(plain, 4),
                             speedup=None if plain is None else round(plain / ms, 2), pow2_decim=None if pow2 is None else pow2[0],
                             k_channelize_grid_ms=None if pow2 is None else round(pow2[1], 4), awgn_tile_ms=round(awgn, 4)))
            del d_out, d_a, d_b
    rx.close()
    print("ratio       M slots   n_out      ms    GB/s  us / slot  direct form ms  speedup  k_channelize_grid D ms  awgn_tile ms")
    for r in rows:
        print("%-7s %5d %5d %7d %7.4f %7.1f %10.3f %15s %8s %13s %9s %13.4f"
              % (r["ratio"], r["m"], r["slots"], r["n_out"], r["ms"], r["gb_per_s"], r["us_per_slot"],
                 "-" if r["direct_ms"] is None else "%.4f" % r["direct_ms"], "-" if r["speedup"] is None else "%.2f" % r["speedup"],
                 "-" if r["pow2_decim"] is None else "%d" % r["pow2_decim"],
                 "-" if r["k_channelize_grid_ms"] is None else "%.4f" % r["k_channelize_grid_ms"], r["awgn_tile_ms"]))
    print(json.dumps({"tool": "channelize_bench", "samples": W, "grid_ratio_rows": rows}), flush=True)


def child_real(args):
    import numpy as np
    import torch
    import modem_amd

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    rx = modem_amd.Receiver(device=0, stream=stream.cuda_stream)
    W = args.samples
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    d_iq = torch.randint(-20000, 20000, (W, 2), dtype=torch.int16, device=dev, generator=gen)
    d_re = d_iq[:, 0].contiguous()

    def timed(f):
        """-> (median, least, most) ms per launch"""
        ms = []
        for k in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.inner):
                f()
            b.record(stream)
            b.synchronize()
            if k >= args.warmup:
                ms.append(a.elapsed_time(b) / args.inner)
        return statistics.median(ms), min(ms), max(ms)

    ratios = []
    for r in args.real:
        for t in (["6", "16", "32"] if r is None else [r]):
            ratios.append(tuple(int(v) for v in t.split("/")) if "/" in t else (int(t), 1))
    rows = []
    for P, Q in ratios:
        decim = P if Q == 1 else (P, Q)
        rw = 8000.0 * P / Q
        n_out = -(-W * Q // P)
        for N in args.channels:
            # inside the real front end's rule, rate / 4 <= |f| <= Rw / 2 - rate / 4, of alternating sign
            f = np.linspace(2000.0 + 1.123, rw / 2 - 2000.0 - 1.123, N) * np.where(np.arange(N) % 2, -1.0, 1.0)
            d_out = torch.empty((N, n_out, 2), dtype=torch.float32, device=dev)
            real = timed(lambda: rx.channelize_real(d_re.data_ptr(), 0, 0, W, decim, f, 0, n_out, d_out.data_ptr()))
            ana = timed(lambda: rx.channelize(d_iq.data_ptr(), 0, 0, W, decim, f, 0, n_out, d_out.data_ptr()))
            rows.append(dict(ratio="%d/%d" % (P, Q), channels=N, n_out=n_out, real_ms=round(real[0], 4), real_min_ms=round(real[1], 4),
                             real_max_ms=round(real[2], 4), analytic_ms=round(ana[0], 4), analytic_min_ms=round(ana[1], 4),
                             analytic_max_ms=round(ana[2], 4), analytic_over_real=round(ana[0] / real[0], 2)))
            del d_out
    rx.close()
    print("ratio   channels   n_out   real ms (least .. most)      analytic ms (least .. most)   analytic / real")
    for r in rows:
        print("%-7s %8d %7d %8.4f (%.4f .. %.4f) %10.4f (%.4f .. %.4f) %12.2f"
              % (r["ratio"], r["channels"], r["n_out"], r["real_ms"], r["real_min_ms"], r["real_max_ms"], r["analytic_ms"], r["analytic_min_ms"],
                 r["analytic_max_ms"], r["analytic_over_real"]))
    print(json.dumps({"tool": "channelize_bench", "samples": W, "inner": args.inner, "reps": args.reps, "real_rows": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--real", action="append", nargs="?", default=[], metavar="P/Q",
                    help="time the front end for a real capture beside the analytic one at D = 6, 16, 32, or at this ratio or D (repeatable)")
    ap.add_argument("--channels", type=int, nargs="+", default=[4, 64], help="channel counts of --real")
    ap.add_argument("--inner", type=int, default=10, help="launches per timed group of --real")
    ap.add_argument("--grid", action="append", nargs="+", default=[], metavar="D", help="time the grid front end at decimation D, or at the ratio P/Q, [SLOTS] (repeatable)")
    ap.add_argument("--ratio", action="append", default=[], metavar="P/Q", help="time the front end at this rational decimation (repeatable)")
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds the GPU step may take")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        if args.real:
            return child_real(args)
        if args.grid and any("/" in g[0] for g in args.grid):
            if not all("/" in g[0] for g in args.grid):
                print("channelize_bench: --grid takes either ratios P/Q or powers of two in one run", file=sys.stderr)
                return 2
            return child_grid_ratio(args)
        return child_grid(args) if args.grid else child_ratio(args) if args.ratio else child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--samples", str(args.samples), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    for r in args.ratio:
        cmd += ["--ratio", r]
    for r in args.real:
        cmd += ["--real"] + ([] if r is None else [r])
    if args.real:
        cmd += ["--inner", str(args.inner), "--channels"] + [str(n) for n in args.channels]
    for g in args.grid:
        cmd += ["--grid"] + g
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print("channelize_bench: the GPU step ran into its time limit of %d s" % args.timeout, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
