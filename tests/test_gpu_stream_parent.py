"""The one-call stream decode is a batch of one recording: both of its entries against what the entry's own driver
and kernel forms returned in the last commit that had them (stream_fixture.py), and - on one handle - between two batched calls,
whose scratch it shares."""
import numpy as np
import pytest

import stream_fixture as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rxs():
    import modem_amd
    made = {}

    def get(rate):
        if rate not in made:
            made[rate] = modem_amd.Receiver(device=0, chunk_frames=16, sample_rate=rate)
        return made[rate]
    yield get
    for r in made.values():
        r.close()


def _device_entry(rx, pcm, cap):
    import torch
    import modem_amd.ofdmrx as M
    d_pcm = torch.from_numpy(np.array(pcm)).cuda()
    d_out = torch.zeros((cap, M.PAYLOAD_BYTES), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((cap, M.RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = rx.decode_stream_device(d_pcm.data_ptr(), rx._fmt(pcm.dtype), pcm.shape[1], len(pcm), cap, d_out.data_ptr(), d_res.data_ptr())
    rx.synchronize()
    k = min(n, cap)
    return d_out.cpu().numpy()[:k], d_res.cpu().numpy()[:k].view(M.RESULT_DTYPE).ravel(), n


@pytest.mark.parametrize("name", ["mixed_2ch", "mixed_mono", "two_44k_mono", "one_48k_2ch", "mixed_u8", "mixed_f32"])
def test_one_call_equals_parent(rxs, name):
    """host entry and device entry, byte for byte"""
    rate, pcm = F.cases()[name]
    rx = rxs(rate)
    F.check(name, pcm, rx.decode_stream(pcm))
    F.check(name, pcm, _device_entry(rx, pcm, 16))


@pytest.mark.parametrize("kind", ["2ch", "mono"])
def test_one_call_between_batched_calls(rxs, kind):
    """three different recordings in one batched call, a one-call decode of the shortest, the batched call again: the lengths, tile
    places, counts and edge shares one call leaves in the handle's scratch are not the next call's"""
    rx = rxs(8000)
    names = ["mixed_" + kind, "three_" + kind, "mirror_" + kind]
    pcms = [F.cases()[n][1] for n in names]
    for n, pcm, got in zip(names, pcms, rx.decode_streams(pcms)):
        F.check(n, pcm, got)
    F.check(names[1], pcms[1], rx.decode_stream(pcms[1]))
    for n, pcm, got in zip(names, pcms, rx.decode_streams(pcms)):
        F.check(n, pcm, got)
    F.check(names[0], pcms[0], rx.decode_stream(pcms[0]))
