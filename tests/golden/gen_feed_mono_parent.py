#!/usr/bin/env python3
"""Record tests/golden/feed_mono_parent.json: what ofdmrx_feed_* returns for the mono cases of tests/feed_fixture.py.

Meant for ONE checkout: the last commit whose feed had a driver and kernel forms of its own (api_feed.cpp, the single-window forms of
k_stream.hip / k_sync.hip).  From the next commit on a feed is a bank of one channel, and a recording made there would hold the bank
to itself; the tests hold the feed and every bank channel to this file instead.  Needs a GPU and the built library.

    python tests/golden/gen_feed_mono_parent.py --commit $(git rev-parse HEAD) [--out FILE]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "feed_mono_parent.json"))
    a = ap.parse_args()
    import bank_inputs as B
    import feed_fixture as F
    import modem_amd
    rxs, cases = {}, {}
    for name, (rate, samples, pushes) in F.cases().items():
        if rate not in rxs:
            rxs[rate] = modem_amd.Receiver(device=0, chunk_frames=16, sample_rate=rate)
        got = B.run_feed(rxs[rate], samples, pushes)
        cases[name] = F.encode(rate, samples, pushes, got)
        print(name, len(samples), "samples,", len(pushes), "pushes,", len(got[1]), "records")
    for r in rxs.values():
        r.close()
    with open(a.out, "w") as f:
        json.dump({"recorded_from_commit": a.commit, "entry": "ofdmrx_feed_begin / _push / _end, chunk_frames 16", "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
