"""The wideband loop through a REAL capture on the device, at 6 and at 25/4: payloads -> tx_encode (2
channels, freq_off 0) -> synthesize to F32 (two channels with distinct |centre|, one of them negative, starts the decimation does not
divide) -> the I component kept on the device, plus real noise -> the real wideband bank and ofdmrx_util_channelize_real ->
payloads.  The real part of a capture synthesized at gain g holds each signal at g / 2 on either side of 0, and the real front end
doubles: a unity round trip.  The capture is copied out once for the checks."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

RATE = 8000
CENTRES = np.array([-14000.0, 9000.0])
GAINS = (0.05, 0.2)
STARTS = (7, 50021)
SIGMA = 1e-3
RATIOS = {"6": (6, 1), "25/4": (25, 4)}


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


@pytest.fixture(scope="module")
def loops(rx):
    """per ratio: the real capture made on the device, its channel rows from the device and their stream decode: computed once"""
    import modem_amd
    import torch
    pays = np.stack([O.payload_for(60 + c) for c in range(2)])
    n_in = rx.tx_frame_samples(6)
    d_pay = torch.from_numpy(pays).to("cuda:0")
    d_pcm = torch.zeros((2, n_in, 2), dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    for c in range(2):
        rx.tx_encode(d_pay[c].data_ptr(), 1, d_pcm[c].data_ptr(), mode=6, freq_off=0, channels=2)
    rx.synchronize()
    frames = d_pcm.cpu().numpy()
    own = [(int(r[1][0]["sc_start"]), float(((f.astype(np.float64) / 32767.0) ** 2).sum())) for r, f in zip(rx.decode_streams(list(frames)), frames)]
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(425)
    out = {}
    for name, (P, Q) in RATIOS.items():
        assert all(s % P for s in STARTS)
        decim = P if Q == 1 else (P, Q)
        W = max(STARTS) + modem_amd.synthesize_support(n_in, decim)
        d_cap = torch.full((W + 1, 2), 12345.0, dtype=torch.float32, device="cuda:0")
        rx.synthesize(d_pcm.data_ptr(), 0, n_in, decim, CENTRES, STARTS, GAINS, 0, W, d_cap.data_ptr(), 2)
        rx.synchronize()
        assert (d_cap[W] == 12345.0).all().item()
        d_real = (d_cap[:W, 0] + SIGMA * torch.randn(W, generator=gen, dtype=torch.float32, device="cuda:0")).contiguous()
        n_out = -(-W * Q // P)
        d_rows = torch.full((2, n_out, 2), 12345.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        rx.channelize_real(d_real.data_ptr(), 2, 0, W, decim, CENTRES, 0, n_out, d_rows.data_ptr())
        rx.synchronize()
        cap, rows = d_real.cpu().numpy(), d_rows.cpu().numpy()
        recs = rx.decode_streams(list(rows))
        for a in (cap, rows):
            a.setflags(write=False)
        out[name] = (decim, cap, rows, recs)
    return pays, own, out


@pytest.mark.parametrize("name", list(RATIOS))
def test_every_frame_decodes_from_its_channel(loops, name):
    pays, own, out = loops
    decim, cap, rows, recs = out[name]
    P, Q = RATIOS[name]
    for c in range(2):
        o, res, npre = recs[c]
        ok = [k for k in range(len(res)) if int(res[k]["status"]) == 0]
        assert len(ok) == 1, (c, [int(s) for s in res["status"]])
        k = ok[0]
        assert (o[k] == pays[c]).all() and int(res[k]["bit_flips"]) == 0 and int(res[k]["oper_mode"]) == 6
        assert abs(int(res[k]["sc_start"]) - (own[c][0] + 24 + STARTS[c] * Q / P)) <= 1, (c, int(res[k]["sc_start"]), own[c])
        # a unity round trip: the row's energy is the transmitted frame's at gain g (no doubling would leave a quarter of it); the
        # noise and the other channel's stop-band leak add a few per cent at the weak channel
        ratio = float((rows[c].astype(np.float64) ** 2).sum()) / (GAINS[c] ** 2 * own[c][1])
        print("%s channel %d: row energy / (g^2 x frame energy) %.4f" % (name, c, ratio))
        assert 0.8 < ratio < 1.25, (c, ratio)


def _by_channel(parts, n_channels):
    pay = np.concatenate([p[0] for p in parts])
    res = np.concatenate([p[1] for p in parts])
    ch = np.concatenate([p[2] for p in parts])
    ix = np.concatenate([p[3] for p in parts])
    return [(pay[ch == c].tobytes(), res[ch == c].tobytes(), list(ix[ch == c])) for c in range(n_channels)]


@pytest.mark.parametrize("blocks", [(1 << 26,), (50000,), (48000, 4097, 1, 0, 5, 7 * 4096 + 3)], ids=["one push", "50000", "mixed"])
@pytest.mark.parametrize("name", list(RATIOS))
def test_real_bank_equals_the_one_call_decode(rx, loops, name, blocks):
    """the capture pushed in blocks (a seam inside every frame) through the real wideband bank gives, per channel and byte for byte, the
    payloads and results of the one-call decode of ofdmrx_util_channelize_real's rows"""
    pays, own, out = loops
    decim, cap, rows, recs = out[name]
    bank = rx.wideband_real_bank(CENTRES, decim, dtype=np.float32)
    parts, at, i = [], 0, 0
    try:
        while at < len(cap):
            n = min(blocks[i % len(blocks)], len(cap) - at)
            parts.append(bank.push(cap[at:at + n]))
            at += n
            i += 1
        parts.append(bank.end())
    finally:
        while bank.open:
            bank.end()
    got = _by_channel(parts, 2)
    for c, (o, res, npre) in enumerate(recs):
        assert got[c][2] == list(range(npre)), c
        assert got[c][0] == o.tobytes() and got[c][1] == res.tobytes(), c


@pytest.mark.parametrize("name", list(RATIOS))
def test_oracle_on_the_rows_agrees(loops, name):
    """the oracle's decoder on the device's rows: every record agrees in status, payload and sc_start"""
    pays, own, out = loops
    decim, cap, rows, recs = out[name]
    for c in range(2):
        o, res, npre = recs[c]
        assert npre >= 1
        for k in range(npre + 1):
            oo, r = O.decode(rows[c], skip=k)
            if k == npre:
                assert r.status == 1
                break
            assert r.status == int(res[k]["status"]) and (oo == o[k]).all() and r.sc_start == int(res[k]["sc_start"]), (c, k)
