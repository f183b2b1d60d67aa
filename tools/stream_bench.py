#!/usr/bin/env python3
"""stream_bench.py -- ofdmrx_decode_stream_device on long recordings, against the batch entry on the same payloads.

Input (made on the device): --streams streams of --count mode-6 payloads each, 8 kHz, 2-channel int16, by the device transmitter
(ofdmrx_tx_encode_stream_device) + ofdmrx_util_awgn_tile at --noise-db.  Timed: one decode_stream_device call per stream per step
(host clock around a synchronise), warm-up first.  Compared in the same process: the batch entry on the same payloads as single-payload
frames (ofdmrx_tx_encode_device, what bench.py runs), and today's route to the payloads of one --skip-count-payload stream (that many
copies of it with skip counts 0 .. n-1).  Every payload is checked.  Prints one JSON line (and writes it to --out).

--feed BLOCK: instead, ONE such recording from host memory through the live feed (ofdmrx_feed_*) in pushes of BLOCK samples, beside the
host-pointer one-call entry (ofdmrx_decode_stream) on the same samples: samples/s and records/s of both and their ratio.  Every push
synchronises with the host, so the feed is the slower per sample; records and payloads are checked to be the same.  feed_ms_per_push*
is a whole run (begin to end) divided by its pushes, feed_push_call_ms_* the median time of one push call, both over the steps.

--batched: instead, the --streams recordings (a) through a loop of ofdmrx_decode_stream_device, one call per recording, and (b) through
ONE ofdmrx_decode_streams_device call, alternating step by step: records/s and samples/s of both with the median and the range over the
steps, and their ratio.  The records of (a) and (b) are checked to be the same bytes.

--bank N BLOCK: N live channels of the same --count payload recording behind staggered leading silence, pushed BLOCK samples per channel
per round through ONE bank (ofdmrx_bank_*), against (a) the only way without it: N handles (chunk_frames 4), each with its own feed,
pushed in a loop (--feeds-cap M: only the first M channels, when N handles do not fit; reported as measured, never scaled), and (b) one
ofdmrx_decode_streams call over the complete recordings - the floor: it has no liveness.  Wall time per round, records/s, the ratios;
every channel's records are checked against (b).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--noise-db", type=float, default=-30.0)
    ap.add_argument("--skip-count", type=int, default=64)
    ap.add_argument("--out", default="")
    ap.add_argument("--feed", type=int, default=0, metavar="BLOCK", help="the same recording through the live feed in pushes of BLOCK samples")
    ap.add_argument("--batched", action="store_true", help="a loop of one-call decodes over the recordings against one ofdmrx_decode_streams_device call")
    ap.add_argument("--bank", type=int, nargs=2, default=None, metavar=("N", "BLOCK"), help="N live channels through one bank, BLOCK samples per channel per round")
    ap.add_argument("--feeds-cap", type=int, default=0, help="--bank: baseline (a) on the first M channels only (0: all N)")
    a = ap.parse_args()
    import torch
    import modem_amd
    import modem_amd.ofdmrx as M
    dev = torch.device("cuda:0")
    rx = modem_amd.Receiver(device=0)
    L = rx._lib
    L.ofdmrx_tx_encode_stream_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    L.ofdmrx_stream_samples.restype = C.c_long
    S, K = a.streams, a.count
    n = int(L.ofdmrx_stream_samples(8000, 6, K))
    if a.batched:
        return batched_bench(a, rx, torch, dev, S, K, n)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    pay = torch.randint(0, 256, (S, K, 5380), dtype=torch.uint8, device=dev, generator=g)
    clean = torch.empty((n, 2), dtype=torch.int16, device=dev)
    pcm = [torch.empty((n, 2), dtype=torch.int16, device=dev) for _ in range(S)]
    for s in range(S):
        rc = L.ofdmrx_tx_encode_stream_device(rx._h, pay[s].data_ptr(), 1, K, 6, 2000, b"ANONYMOUS", 2, 16, clean.data_ptr())
        assert rc == 0, rc
        rx.awgn_tile(clean.data_ptr(), 1, pcm[s].data_ptr(), 1, n, a.noise_db, 11 + s, 0)
    rx.synchronize()
    del clean
    if a.feed:
        return feed_bench(a, rx, pcm[0].cpu().numpy(), pay[0].cpu().numpy())
    if a.bank:
        return bank_bench(a, rx, pcm[0].cpu().numpy(), pay[0].cpu().numpy())
    out = torch.zeros((S, K, 5380), dtype=torch.uint8, device=dev)
    res = torch.zeros((S, K, M.RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)

    def stream_step():
        for s in range(S):
            npre = rx.decode_stream_device(pcm[s].data_ptr(), 0, 2, n, K, out[s].data_ptr(), res[s].data_ptr())
            assert npre == K, npre
        rx.synchronize()

    for _ in range(a.warmup):
        stream_step()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        stream_step()
    dt = (time.perf_counter() - t0) / a.steps
    tm = rx.timing()
    ok = int((out == pay).all(dim=2).sum().item())
    status = res.cpu().numpy().reshape(S * K, -1).view(M.RESULT_DTYPE).ravel()["status"]
    stream_fps = S * K / dt
    # the batch entry on the same payloads as single-payload frames
    spf = int(L.ofdmrx_tx_frame_samples(6))
    clean = torch.empty((S * K, spf, 2), dtype=torch.int16, device=dev)
    rx.tx_encode(pay.reshape(S * K, 5380).data_ptr(), S * K, clean.data_ptr(), mode=6, channels=2)
    frames = torch.empty_like(clean)
    rx.awgn_tile(clean.data_ptr(), S * K, frames.data_ptr(), S * K, spf, a.noise_db, 11, 0)
    del clean
    bout = torch.zeros((S * K, 5380), dtype=torch.uint8, device=dev)
    bres = torch.zeros((S * K, M.RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    for _ in range(a.warmup):
        rx.decode_device(frames.data_ptr(), 0, 2, spf, spf * 4, S * K, bout.data_ptr(), bres.data_ptr())
        rx.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        rx.decode_device(frames.data_ptr(), 0, 2, spf, spf * 4, S * K, bout.data_ptr(), bres.data_ptr())
        rx.synchronize()
    bdt = (time.perf_counter() - t0) / a.steps
    bok = int((bout == pay.reshape(S * K, 5380)).all(dim=1).sum().item())
    del frames, bout, bres
    # today's route to the payloads of one stream: copies of it with skip counts 0 .. n-1
    J = a.skip_count
    nj = int(L.ofdmrx_stream_samples(8000, 6, J))
    clean = torch.empty((nj, 2), dtype=torch.int16, device=dev)
    L.ofdmrx_tx_encode_stream_device(rx._h, pay[0, :J].contiguous().data_ptr(), 1, J, 6, 2000, b"ANONYMOUS", 2, 16, clean.data_ptr())
    one = torch.empty_like(clean)
    rx.awgn_tile(clean.data_ptr(), 1, one.data_ptr(), 1, nj, a.noise_db, 11, 0)
    copies = one[None].repeat(J, 1, 1).contiguous()
    skips = torch.arange(J, dtype=torch.int32, device=dev)
    sout = torch.zeros((J, 5380), dtype=torch.uint8, device=dev)
    sres = torch.zeros((J, M.RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    rx.decode_device(copies.data_ptr(), 0, 2, nj, nj * 4, J, sout.data_ptr(), sres.data_ptr(), d_skip=skips.data_ptr())
    rx.synchronize()
    t0 = time.perf_counter()
    rx.decode_device(copies.data_ptr(), 0, 2, nj, nj * 4, J, sout.data_ptr(), sres.data_ptr(), d_skip=skips.data_ptr())
    rx.synchronize()
    sdt = time.perf_counter() - t0
    sok = int((sout == pay[0, :J]).all(dim=1).sum().item())
    sstat = np.bincount(sres.cpu().numpy().view(M.RESULT_DTYPE).ravel()["status"], minlength=7).tolist()
    t1 = time.perf_counter()
    npre = rx.decode_stream_device(one.data_ptr(), 0, 2, nj, J, sout.data_ptr(), sres.data_ptr())
    rx.synchronize()
    s1dt = time.perf_counter() - t1
    s1ok = int((sout == pay[0, :J]).all(dim=1).sum().item())
    rec = {
        "metric": "stream decode, mode-6 8 kHz 2-channel int16, AWGN %g dB" % a.noise_db,
        "streams": S, "payloads_per_stream": K, "samples_per_stream": n, "steps": a.steps,
        "stream_ms_per_step": dt * 1e3, "stream_frames_per_s": stream_fps, "stream_payloads_ok": ok, "stream_status_ok": int((status == 0).sum()),
        "stream_stage_ms_last_call": {k: round(v[0], 3) for k, v in tm.items()},
        "batch_ms_per_step": bdt * 1e3, "batch_frames_per_s": S * K / bdt, "batch_payloads_ok": bok,
        "stream_vs_batch": stream_fps / (S * K / bdt),
        "skip_route_payloads": J, "skip_route_ms": sdt * 1e3, "skip_route_frames_per_s": J / sdt, "skip_route_payloads_ok": sok, "skip_route_status_counts": sstat,
        "stream_route_same_payloads_ms": s1dt * 1e3, "stream_route_preambles": npre, "stream_route_payloads_ok": s1ok,
        "input_bytes_per_step": S * n * 4,
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    rx.close()


def batched_bench(a, rx, torch, dev, S, K, n):
    """S recordings of K payloads: a loop of one-call decodes against one call for all of them"""
    import modem_amd.ofdmrx as M
    L = rx._lib
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    pay = torch.randint(0, 256, (S, K, 5380), dtype=torch.uint8, device=dev, generator=g)
    clean = torch.empty((S, n, 2), dtype=torch.int16, device=dev)
    pcm = torch.empty((S, n, 2), dtype=torch.int16, device=dev)
    rc = L.ofdmrx_tx_encode_stream_device(rx._h, pay.data_ptr(), S, K, 6, 2000, b"ANONYMOUS", 2, 16, clean.data_ptr())
    assert rc == 0, rc
    rx.awgn_tile(clean.data_ptr(), S, pcm.data_ptr(), S, n, a.noise_db, 11, 0)
    rx.synchronize()
    del clean
    rsz = M.RESULT_DTYPE.itemsize
    outs = {k: (torch.zeros((S * K, 5380), dtype=torch.uint8, device=dev), torch.zeros((S * K, rsz), dtype=torch.uint8, device=dev)) for k in ("loop", "batched")}
    lens = np.full(S, n, np.uintp)

    def loop():
        out, res = outs["loop"]
        for s in range(S):
            npre = rx.decode_stream_device(pcm[s].data_ptr(), 0, 2, n, K, out[s * K].data_ptr(), res[s * K].data_ptr())
            assert npre == K, npre
        rx.synchronize()

    def batched():
        out, res = outs["batched"]
        npre, first = rx.decode_streams_device(pcm.data_ptr(), 0, 2, lens, n * 4, K, S * K, out.data_ptr(), res.data_ptr())
        rx.synchronize()
        assert (npre == K).all() and first[S] == S * K, (npre, first)

    for _ in range(a.warmup):
        loop()
        batched()
    times = {"loop": [], "batched": []}
    for _ in range(a.steps):                                     # alternating: both see the same drift of the clocks
        for name, fn in (("loop", loop), ("batched", batched)):
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    same = all(bool((outs["loop"][i] == outs["batched"][i]).all().item()) for i in (0, 1))
    ok = int((outs["batched"][0] == pay.reshape(S * K, 5380)).all(dim=1).sum().item())
    rec = {"metric": "many recordings: a loop of ofdmrx_decode_stream_device against one ofdmrx_decode_streams_device, mode-6 8 kHz 2-channel int16, "
                     "AWGN %g dB" % a.noise_db,
           "streams": S, "payloads_per_stream": K, "samples_per_stream": n, "steps": a.steps, "warmup": a.warmup}
    for name in ("loop", "batched"):
        t = np.array(times[name])
        med = float(np.median(t))
        rec.update({name + "_ms_median": med * 1e3, name + "_ms_min": float(t.min()) * 1e3, name + "_ms_max": float(t.max()) * 1e3,
                    name + "_records_per_s": S * K / med, name + "_samples_per_s": S * n / med})
    rec.update({"batched_vs_loop": rec["loop_ms_median"] / rec["batched_ms_median"],
                "batched_vs_loop_worst_case": rec["loop_ms_min"] / rec["batched_ms_max"],
                "same_bytes_as_loop": same, "payloads_ok": ok})
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    rx.close()


def feed_bench(a, rx, pcm, pay):
    """one recording (host memory): the one-call host entry against the feed in pushes of a.feed samples"""
    n, K, B = len(pcm), len(pay), a.feed

    def one_call():
        return rx.decode_stream(pcm, max_frames=K)[:2]

    push_medians = []                                            # per run of the feed: the median time of one push call

    def fed():
        got, t_push = [], []
        with rx.feed(2) as f:
            for p in range(0, n, B):
                t0 = time.perf_counter()
                got.append(f.push(pcm[p:p + B]))
                t_push.append(time.perf_counter() - t0)
            got.append(f.end())
        push_medians.append(float(np.median(t_push)))
        return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])

    times, per_step = {}, {}
    outs = {}
    for name, fn in (("one_call", one_call), ("feed", fed)):
        for _ in range(a.warmup):
            fn()
        per_step[name] = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            outs[name] = fn()
            per_step[name].append(time.perf_counter() - t0)
        times[name] = float(np.mean(per_step[name]))
    same = outs["feed"][0].tobytes() == outs["one_call"][0].tobytes() and outs["feed"][1].tobytes() == outs["one_call"][1].tobytes()
    rec = {
        "metric": "live feed against the one-call host entry, mode-6 8 kHz 2-channel int16, AWGN %g dB" % a.noise_db,
        "payloads": K, "samples": n, "block": B, "pushes": (n + B - 1) // B, "steps": a.steps,
        "one_call_ms": times["one_call"] * 1e3, "one_call_samples_per_s": n / times["one_call"], "one_call_records_per_s": K / times["one_call"],
        "feed_ms": times["feed"] * 1e3, "feed_samples_per_s": n / times["feed"], "feed_records_per_s": len(outs["feed"][1]) / times["feed"],
        "feed_vs_one_call": times["one_call"] / times["feed"], "feed_ms_per_push": times["feed"] * 1e3 / ((n + B - 1) // B),
        "feed_ms_per_push_median": float(np.median(per_step["feed"])) * 1e3 / ((n + B - 1) // B),
        "feed_ms_per_push_min": min(per_step["feed"]) * 1e3 / ((n + B - 1) // B), "feed_ms_per_push_max": max(per_step["feed"]) * 1e3 / ((n + B - 1) // B),
        "feed_push_call_ms_median": float(np.median(push_medians[-a.steps:])) * 1e3, "feed_push_call_ms_min": min(push_medians[-a.steps:]) * 1e3,
        "feed_push_call_ms_max": max(push_medians[-a.steps:]) * 1e3,
        "records": len(outs["feed"][1]), "payloads_ok": int((outs["feed"][0] == pay).all(axis=1).sum()), "same_bytes_as_one_call": bool(same),
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    rx.close()


def bank_bench(a, rx, pcm, pay):
    """N live channels of one recording behind staggered silence: one bank against N feeds in a loop and against one decode_streams call"""
    import modem_amd
    N, B = a.bank
    K = len(pay)
    leads = [(c * 997) % 8000 for c in range(N)]
    chans = [np.concatenate([np.zeros((lead, 2), np.int16), pcm]) for lead in leads]
    longest = max(len(c) for c in chans)
    rounds = (longest + B - 1) // B

    def floor():
        return rx.decode_streams(chans)

    def bank():
        per = [[] for _ in range(N)]
        t_round = []
        with rx.bank(N, 2) as b:
            for r in range(rounds):
                t0 = time.perf_counter()
                o, res, rc, ri = b.push([c[r * B:(r + 1) * B] for c in chans])
                t_round.append(time.perf_counter() - t0)
                for c in np.unique(rc):
                    per[c].append((o[rc == c], res[rc == c]))
            o, res, rc, ri = b.end()
            for c in np.unique(rc):
                per[c].append((o[rc == c], res[rc == c]))
        return per, t_round

    M = a.feeds_cap or N
    rxs = [modem_amd.Receiver(device=0, chunk_frames=4) for _ in range(M)]

    def feeds():
        per = [[] for _ in range(M)]
        t_round = []
        fs = [r.feed(2) for r in rxs]
        for r in range(rounds):
            t0 = time.perf_counter()
            for c in range(M):
                per[c].append(fs[c].push(chans[c][r * B:(r + 1) * B]))
            t_round.append(time.perf_counter() - t0)
        for c in range(M):
            per[c].append(fs[c].end())
            while fs[c].open:
                fs[c].end()
        return per, t_round

    def joined(parts):
        return (np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, 5380), np.uint8),
                np.concatenate([p[1] for p in parts]) if parts else np.zeros(0))

    res = {}
    for name, fn in (("bank", bank), ("feeds", feeds)):
        for _ in range(a.warmup):
            fn()
        walls, per_round = [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            out, t_round = fn()
            walls.append(time.perf_counter() - t0)
            per_round.append(float(np.median(t_round)))
        res[name] = (out, walls, per_round)
    for _ in range(a.warmup):
        floor()
    fl_walls = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        want = floor()
        fl_walls.append(time.perf_counter() - t0)
    same_bank = all(joined(res["bank"][0][c])[0].tobytes() == want[c][0].tobytes() and joined(res["bank"][0][c])[1].tobytes() == want[c][1].tobytes()
                    for c in range(N))
    same_feeds = all(joined(res["feeds"][0][c])[0].tobytes() == want[c][0].tobytes() for c in range(M))
    n_rec = sum(len(w[1]) for w in want)
    med = lambda v: float(np.median(v))
    bank_wall, feeds_wall = med(res["bank"][1]), med(res["feeds"][1])
    rec = {
        "metric": "live feed bank: N channels of one recording, mode-6 8 kHz 2-channel int16, AWGN %g dB, against N feeds and one decode_streams call" % a.noise_db,
        "channels": N, "block": B, "payloads_per_channel": K, "rounds": rounds, "steps": a.steps, "warmup": a.warmup, "records": n_rec,
        "bank_ms_per_round_median": med(res["bank"][2]) * 1e3, "bank_ms_per_round_min": min(res["bank"][2]) * 1e3,
        "bank_ms_per_round_max": max(res["bank"][2]) * 1e3, "feeds_ms_per_round_min": min(res["feeds"][2]) * 1e3,
        "feeds_ms_per_round_max": max(res["feeds"][2]) * 1e3, "bank_wall_ms_median": bank_wall * 1e3, "bank_wall_ms_min": min(res["bank"][1]) * 1e3,
        "bank_wall_ms_max": max(res["bank"][1]) * 1e3, "bank_records_per_s": n_rec / bank_wall,
        "feeds_channels": M, "feeds_ms_per_round_median": med(res["feeds"][2]) * 1e3, "feeds_wall_ms_median": feeds_wall * 1e3,
        "feeds_wall_ms_min": min(res["feeds"][1]) * 1e3, "feeds_wall_ms_max": max(res["feeds"][1]) * 1e3,
        "feeds_records_per_s": n_rec * M / N / feeds_wall,
        "bank_vs_feeds_per_channel": (feeds_wall / M) / (bank_wall / N),
        "one_call_wall_ms_median": med(fl_walls) * 1e3, "one_call_records_per_s": n_rec / med(fl_walls), "bank_vs_one_call": med(fl_walls) / bank_wall,
        "bank_same_bytes_as_one_call": bool(same_bank), "feeds_same_payloads_as_one_call": bool(same_feeds),
        "payloads_ok": int(sum((w[0][:K] == pay).all(axis=1).sum() for w in want)),
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    for r in rxs:
        r.close()
    rx.close()


if __name__ == "__main__":
    main()
