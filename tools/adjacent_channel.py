#!/usr/bin/env python3
"""Adjacent-channel interference on the device: a victim transmission at the centre of a wideband capture
with one neighbour `spacing` Hz below it and one above, both `level` dB above the victim.  The whole loop stays in HBM:
  tx_encode at freq_off 0 (victim and neighbours, different payloads) -> synthesize (interp x the handle's rate, the neighbours
  started 7 and 13 wideband samples late) -> awgn_tile on the capture -> channelize at the victim's centre -> decode_streams_device.
A victim frame counts as received when a record of status 0 carries its payload.  For every spacing and level it prints one JSON line
  {"spacing_hz", "level_db", "frames", "fer", "ber", "records"}   (ber: over the frames that gave a record where they were sent)
and at the end one line with all of them.  --ratio P/Q runs the same loop at a rational capture rate (section 4.18: synthesize and
channelize take the ratio, the capture is at rate x P / Q); without it nothing changes.  The victim's gain is chosen so that the three signals together stay inside int16.
The GPU work runs in a child process under a time limit; the parent never opens the GPU."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def point(rx, torch, np, M, args, spacing, level, seed):
    dev = torch.device("cuda", 0)
    N = args.frames
    D = args.interp if args.ratio is None else args.ratio               # an int, or the pair (p, q)
    spf = rx.tx_frame_samples(args.mode)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    d_pay = torch.randint(0, 256, (3 * N, 5380), dtype=torch.uint8, device=dev, generator=gen)
    d_pcm = torch.empty((3, N * spf, 2), dtype=torch.int16, device=dev)
    rx.tx_encode(d_pay.data_ptr(), 3 * N, d_pcm.data_ptr(), mode=args.mode, freq_off=0, channels=2)
    ratio = 10.0 ** (level / 20.0)
    g_v = 0.9 / (1.0 + 2.0 * ratio)
    starts = np.array([0, 7, 13], np.int64)
    W = int(starts.max()) + M.synthesize_support(N * spf, D)
    d_cap = torch.empty((W, 2), dtype=torch.int16, device=dev)
    rx.synthesize(d_pcm.data_ptr(), M.FMT_S16, N * spf, D, [0.0, -spacing, spacing], starts, [g_v, g_v * ratio, g_v * ratio], 0, W,
                  d_cap.data_ptr(), M.FMT_S16)
    rx.awgn_tile(d_cap.data_ptr(), 1, d_cap.data_ptr(), 1, W, args.noise_db, seed, 0)
    n_rows = -(-W // D) if args.ratio is None else -(-W * D[1] // D[0])
    d_row = torch.empty((1, n_rows, 2), dtype=torch.float32, device=dev)
    rx.channelize(d_cap.data_ptr(), M.FMT_S16, 0, W, D, [0.0], 0, n_rows, d_row.data_ptr())
    cap = 4 * N + 8
    d_out = torch.zeros((cap, 5380), dtype=torch.uint8, device=dev)
    d_res = torch.zeros((cap, M.RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    npre, first = rx.decode_streams_device(d_row.data_ptr(), M.FMT_F32, 2, [n_rows], n_rows * 8, cap, cap, d_out.data_ptr(), d_res.data_ptr())
    rx.synchronize()
    k = min(int(first[1]), cap)
    out = d_out[:k].cpu().numpy()
    res = d_res[:k].cpu().numpy().view(M.RESULT_DTYPE).reshape(-1)
    pay = d_pay[:N].cpu().numpy()
    good = [bool(((out == pay[i]).all(axis=1) & (res["status"] == 0)).any()) for i in range(N)]
    bits = errs = 0
    for i in range(N):                                                # the record nearest to where frame i was sent, if one is near
        at = i * spf + 24                                              # (the victim starts at 0: its delay is 24 at any ratio)
        near = [j for j in range(k) if 0 <= int(res["sc_start"][j]) - at < spf and res["status"][j] in (0, 6)]
        if near:
            j = near[0]
            errs += int(np.unpackbits(out[j] ^ pay[i]).sum())
            bits += 5380 * 8
    return dict(spacing_hz=spacing, level_db=level, frames=N, fer=1.0 - sum(good) / N, ber=(errs / bits) if bits else None, records=k)


def child(args):
    import numpy as np
    import torch
    import modem_amd
    import modem_amd.ofdmrx as M

    rx = modem_amd.Receiver(device=0, chunk_frames=max(1, min(args.frames, 64)), sample_rate=args.rate)
    rows = []
    try:
        for si, spacing in enumerate(args.spacings):
            for li, level in enumerate(args.levels):
                r = point(rx, torch, np, M, args, float(spacing), float(level), 1000 + 100 * si + li)
                print(json.dumps(r), flush=True)
                rows.append(r)
    finally:
        rx.close()
    print(json.dumps({"tool": "adjacent_channel", "interp": args.interp if args.ratio is None else "%d/%d" % args.ratio, "rate": args.rate, "mode": args.mode, "noise_db": args.noise_db, "rows": rows}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--interp", type=int, default=6)
    ap.add_argument("--ratio", default=None, help="P/Q: a rational capture rate in place of --interp (Q <= 16, 2 <= P / Q <= 32)")
    ap.add_argument("--rate", type=int, default=8000)
    ap.add_argument("--mode", type=int, default=6)
    ap.add_argument("--frames", type=int, default=16, help="victim frames per point")
    ap.add_argument("--spacings", type=float, nargs="+", default=[8000.0, 4000.0, 3600.0, 3200.0, 2800.0, 2400.0])
    ap.add_argument("--levels", type=float, nargs="+", default=[0.0, 20.0, 40.0])
    ap.add_argument("--noise-db", type=float, default=-50.0, help="noise on the capture, dB relative to full scale")
    ap.add_argument("--timeout", type=int, default=300, help="seconds the GPU step may take")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    ratio = args.ratio
    if ratio is not None:
        try:
            p, q = (int(v) for v in ratio.split("/"))
        except ValueError:
            ap.error("--ratio takes P/Q")
        args.ratio = (p, q)
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--interp", str(args.interp), "--rate", str(args.rate), "--mode", str(args.mode),
           "--frames", str(args.frames), "--noise-db", str(args.noise_db), "--spacings"] + [str(s) for s in args.spacings] + ["--levels"] + [
               str(v) for v in args.levels] + ([] if ratio is None else ["--ratio", ratio])
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print("adjacent_channel: the GPU step ran into its time limit of %d s" % args.timeout, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
