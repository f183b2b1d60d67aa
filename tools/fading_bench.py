#!/usr/bin/env python3
"""Time ofdmrx_util_fading beside the two kernels it is measured against, on the same resident buffers.

`--frames` (8192) mode-6 frames at 8 kHz are transmitted on the device once; then, with hipEvents on the handle's stream:
  fading     two paths, the F.520 "poor" preset (k_fading)
  awgn_tile  -30 dB (k_awgn_tile: the same bytes moved, a transcendental per sample as well)
  channel    the two-tap static multipath of the same delays (k_channel; 65535 frames per call at most)
and one transmit + decode step of the same frames, which gives the fraction of a Monte-Carlo step that fading adds.
Prints one JSON line; times are the median of `--reps` runs after `--warmup`.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--preset", default="poor")
    args = ap.parse_args()

    import torch
    import modem_amd
    import modem_amd.ofdmrx as M

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    rx = modem_amd.Receiver(device=0, stream=stream.cuda_stream)
    n, spf = args.frames, rx.tx_frame_samples(6)
    paths = modem_amd.watterson(args.preset, 8000)
    taps = [(d, g) for d, g, _ in paths]
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    d_pay = torch.randint(0, 256, (n, 5380), dtype=torch.uint8, device=dev, generator=gen)
    d_a = torch.empty((n, spf, 2), dtype=torch.int16, device=dev)
    d_b = torch.empty_like(d_a)
    d_out = torch.zeros((n, 5380), dtype=torch.uint8, device=dev)
    d_res = torch.zeros((n, M.RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)

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

    tx_ms = timed(lambda k: rx.tx_encode(d_pay.data_ptr(), n, d_a.data_ptr(), mode=6, freq_off=2000, call_sign="ANONYMOUS", channels=2))
    fading_ms = timed(lambda k: rx.fading(d_a.data_ptr(), n, d_b.data_ptr(), n, spf, paths, 777, k * n))
    awgn_ms = timed(lambda k: rx.awgn_tile(d_a.data_ptr(), n, d_b.data_ptr(), n, spf, -30.0, 777, k * n))
    channel_ms = timed(lambda k: rx.channel(d_a.data_ptr(), d_b.data_ptr(), n, spf, multipath=taps))
    rx.awgn_tile(d_a.data_ptr(), n, d_b.data_ptr(), n, spf, -30.0, 777, 0)
    decode_ms = timed(lambda k: rx.decode_device(d_b.data_ptr(), M.FMT_S16, 2, spf, spf * 4, n, d_out.data_ptr(), d_res.data_ptr()))
    rx.synchronize()
    ok = int((d_res.view(torch.int32)[:, 0] == 0).sum())
    gb = 2.0 * n * spf * 4 / 1e9
    print(json.dumps({"tool": "fading_bench", "frames": n, "samples_per_frame": spf, "preset": args.preset,
                      "fading_ms": round(fading_ms, 3), "awgn_tile_ms": round(awgn_ms, 3), "channel_ms": round(channel_ms, 3),
                      "fading_over_awgn": round(fading_ms / awgn_ms, 3), "fading_gb_per_s": round(gb / (fading_ms * 1e-3), 1),
                      "tx_ms": round(tx_ms, 3), "decode_ms": round(decode_ms, 3), "decoded": ok,
                      "fading_share_of_tx_plus_decode": round(fading_ms / (tx_ms + decode_ms), 4)}), flush=True)
    rx.close()


if __name__ == "__main__":
    main()
