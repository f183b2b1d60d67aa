#!/usr/bin/env python3
"""Generate tests/golden/base_frames_2ch_{0,1}.npz: a few clean mode-6 frames exactly as the oracle's
restatement of `encode OUT 8000 16 2 2000 6 ANONYMOUS payload` writes them (2-channel analytic
int16, 95200 samples) together with their payloads.  bench.py tiles them and adds per-frame AWGN on
the device (config 3 of BASELINE.json); tests use them as known-answer inputs.  Data only.  Two files of two frames each:
every committed file stays under 1 MiB; concatenated in file order they are the four frames."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402

N = 4
pays = np.stack([O.payload_for(9000 + i) for i in range(N)])
pcm = np.stack([O.encode_pcm(pays[i], bits=16, channels=2, freq_off=2000, call_sign="ANONYMOUS", mode=6) for i in range(N)])
for part in range(2):
    path = os.path.join(HERE, "base_frames_2ch_%d.npz" % part)
    np.savez_compressed(path, pcm=pcm[2 * part:2 * part + 2], payload=pays[2 * part:2 * part + 2])
    print(pcm.shape, pcm.dtype, path, os.path.getsize(path))
