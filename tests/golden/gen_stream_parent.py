#!/usr/bin/env python3
"""Record tests/golden/stream_parent.json: what ofdmrx_decode_stream returns for the cases of tests/stream_fixture.py.

Meant for ONE checkout: the last commit in which the one-call stream decode had a driver and kernel forms of its own (api_stream.cpp,
the FrameBatch forms of k_stream.hip).  From the next commit on the one-call entry is a batch of one recording, and a recording made
there would hold the batched entry to itself; the tests hold both entries to this file instead.  The device entry is run beside the
host entry and must return the same bytes, so one recording stands for both.  Needs a GPU and the built library.

    python tests/golden/gen_stream_parent.py --commit $(git rev-parse HEAD) [--out FILE]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def device_entry(rx, pcm, cap):
    """the recording through ofdmrx_decode_stream_device -> (payloads, results, n_preambles)"""
    import torch
    import modem_amd.ofdmrx as M
    d_pcm = torch.from_numpy(pcm.copy()).cuda()
    d_out = torch.zeros((max(cap, 1), M.PAYLOAD_BYTES), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((max(cap, 1), M.RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = rx.decode_stream_device(d_pcm.data_ptr(), rx._fmt(pcm.dtype), pcm.shape[1], len(pcm), cap, d_out.data_ptr(), d_res.data_ptr())
    rx.synchronize()
    k = min(n, cap)
    return d_out.cpu().numpy()[:k], d_res.cpu().numpy()[:k].view(M.RESULT_DTYPE).ravel(), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "stream_parent.json"))
    a = ap.parse_args()
    import stream_fixture as F
    import modem_amd
    rxs, cases = {}, {}
    for name, (rate, pcm) in F.cases().items():
        if rate not in rxs:
            rxs[rate] = modem_amd.Receiver(device=0, chunk_frames=16, sample_rate=rate)
        got = rxs[rate].decode_stream(pcm)
        dev = device_entry(rxs[rate], pcm, max(16, got[2]))
        assert dev[2] == got[2] and dev[0].tobytes() == got[0].tobytes() and dev[1].tobytes() == got[1].tobytes(), name
        cases[name] = F.encode(rate, pcm, got)
        print(name, pcm.shape, pcm.dtype, got[2], "preambles,", len(got[1]), "records")
    for r in rxs.values():
        r.close()
    with open(a.out, "w") as f:      # one record per line
        head = {"recorded_from_commit": a.commit, "entry": "ofdmrx_decode_stream (ofdmrx_decode_stream_device: the same bytes), chunk_frames 16"}
        f.write("{\n" + "".join(" %s: %s,\n" % (json.dumps(k), json.dumps(v)) for k, v in head.items()) + ' "cases": {\n')
        for i, (name, c) in enumerate(cases.items()):
            recs = c.pop("records")
            f.write("  %s: {%s, \"records\": [\n" % (json.dumps(name), json.dumps(c)[1:-1]))
            f.write(",\n".join("   " + json.dumps(r) for r in recs))
            f.write("\n  ]}%s\n" % ("," if i + 1 < len(cases) else ""))
        f.write(" }\n}\n")


if __name__ == "__main__":
    main()
