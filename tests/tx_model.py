"""A float64 model of the transmitter (Encoder<value,cmplx,rate> and main()'s payload handling, encode.cc:27-318, 337-445) -- TEST
INFRASTRUCTURE.  It judges oracle/encoder.c and modem_amd/csrc/k_tx.hip by their PCM, sample by sample.

Integer stages come from the oracle's helpers, which test_oracle_kat.py pins: scramble, CRC-32, orc_polar_sysenc, BCH parity, CRC-16,
the MLS generators, base-37.  Everything with a float in it is float64 numpy, restated from encode.cc (cited by line), not from
oracle/encoder.c: carrier amplitudes, the differential products of header and rows, the 4x oversampled PAPR clip, the symbol
transform and its scale, the cross-fade, the silences, the quantiser's clamp and scale.  The model's own error (numpy's transforms
of at most 30720 points, a product of at most 126 unit factors per carrier) is below 1e-9 LSB.

The rule is noise_model.explain / accept as they stand: a sample is explained if it equals rint(v), or is 1 off with the unrounded v
within the tolerance of the rounding boundary between the two; nothing may be unexplained, and at most CAP = 1 % of a comparison
may be off rint(v).

The tolerance is a measurement.  MEASURED_FS is the oracle's worst boundary distance against this model over the whole case table
(cases(), every stream of every case), in units of full scale: the largest |v - boundary| among the oracle's samples that are 1 off
rint(v).  test_tx_model_cpu.py re-measures it on every run (it may not exceed the constant, nor fall below half of it) and
profiles/tx_parity.txt records it case by case.  TOL_FS = 4 x MEASURED_FS, shared by 8-bit and 16-bit output (as a fraction of full
scale; in LSB it is TOL_FS x 32767 or x 127).  Why 4: the device runs a different fp32 factorisation of the same depth - four
decimated N-point transform pairs plus a twiddle combine where the oracle runs one 4N-point pair, Markstein quotients where the
oracle divides - so its errors have about the oracle's sigma; the worst of the table's ~1e7 roughly Gaussian errors already sits
near 5 sigma, and 4 x covers twice the sigma with room for the tail.  The condition on whatever is measured: TOL_FS x 32767 must
stay below 0.25 LSB of 16 bit, or an "explained" sample proves little.

  MEASURED_FS = 8.76e-7   (8.750e-7 rounded up: 0.0287 LSB of 16 bit, in "A mode 11", 8 kHz at -2800 Hz; profiles/tx_parity.txt)
  TOL_FS      = 3.504e-6  (0.115 LSB of 16 bit, 0.00045 LSB of 8 bit)

`variant=` makes the model wrong in one named way (VARIANTS) for the teeth tests; it has no other use."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

import oracle_lib as O

MEASURED_FS = 8.76e-7
TOL_FS = 4.0 * MEASURED_FS
DATA_BITS = 43040                                 # encode.cc:33
CRC_BITS = DATA_BITS + 32                         # encode.cc:35
MLS0_LEN, MLS0_POLY = 127, 0b10001001             # encode.cc:36-37
MLS1_LEN, MLS1_POLY = 255, 0b100101011            # encode.cc:38-39
MLS2_POLY = 0b100101010001                        # encode.cc:40
RATES = (8000, 16000, 44100, 48000)               # encode.cc:424-436

# encode.cc:199-266 (prepare) and 363-387 (band_width): mode -> cons_cols, mod_bits, cons_bits, mesg_bits, frozen table, band width
Mode = namedtuple("Mode", "cols mod_bits cons_bits mesg_bits table band_width")
MODES = {6: Mode(432, 3, 64800, 43808, 0, 2700), 7: Mode(400, 3, 64800, 43808, 0, 2500), 8: Mode(400, 2, 64800, 43808, 0, 2500),
         9: Mode(360, 2, 64800, 43808, 0, 2250), 10: Mode(512, 3, 64512, 44096, 1, 3200), 11: Mode(384, 3, 64512, 44096, 1, 2400),
         12: Mode(384, 2, 64512, 44096, 1, 2400), 13: Mode(256, 2, 64512, 44096, 1, 1600)}

VARIANTS = ("ramp i/guard_len", "guard from the wrong end", "tail forgotten at a payload boundary", "clip by |v|", "papr on schmidl-cox",
            "no papr on data rows", "spill kept", "offset one bin off", "meta-data unscrambled", "rows multiply the pilot",
            "tail message bits not fixed", "one code bit flipped", "rate - 1 leading silence", "8-bit offset 127", "re and im swapped")


def factor(bits):
    return float((1 << (bits - 1)) - 1)


def tol_lsb(bits):
    return TOL_FS * factor(bits)


def symbol_len(rate):
    return (1280 * rate) // 8000                  # encode.cc:31


def rows_of(mode):
    m = MODES[mode]
    return m.cons_bits // m.mod_bits // m.cols    # encode.cc:267-268


def stream_samples(rate, mode, count):
    sl = symbol_len(rate)
    return 2 * rate + (2 + count * (3 + rows_of(mode))) * (sl + sl // 8)


def offset_range(mode, rate, channels):
    """encode.cc:389 (integer halves as there): the smallest and largest freq_off main() lets through"""
    bw = MODES[mode].band_width
    lo = bw // 2 - rate // 2
    if channels == 1:
        lo = max(lo, bw // 2)
    return lo, rate // 2 - bw // 2


def permitted_offsets(mode, rate, channels):
    """every freq_off that passes encode.cc:389 and 394 (a multiple of 50), ascending; [0] and [-1] are the band edges"""
    lo, hi = offset_range(mode, rate, channels)
    return list(range(-(-lo // 50) * 50, hi + 1, 50))


# ---------------------------------------------------------------- integer stages (the oracle's helpers)
class _Mls(C.Structure):
    _fields_ = [("poly", C.c_int), ("test", C.c_int), ("reg", C.c_int)]


def mls_nrz(poly, n):
    """n outputs of CODE::MLS(poly) as 1 - 2 * bit (encode.cc:76-79)"""
    L, s = O.lib(), _Mls()
    L.orc_mls_init(C.byref(s), poly)
    return np.array([1 - 2 * L.orc_mls_next(C.byref(s)) for _ in range(n)], np.float64)


def _frozen_bits(table):
    fr = O.frozen(table)
    return ((fr[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1).astype(bool)


def code_bits(payload, mode, variant=None):
    """main()'s scrambler and encode.cc:293-303: one payload of 5380 bytes -> the shortened code word, NRZ, [cons_bits]"""
    m, L = MODES[mode], O.lib()
    inp = np.ascontiguousarray(payload, np.uint8).copy()
    L.orc_scramble(O.ptr(inp), O.DATA_BYTES)                                           # encode.cc:417-419
    # encode.cc:300-301: the bits past the CRC are +1 (zero), which is what makes the code a shortened one.  In both frozen tables the
    # positions shorten() then removes are exactly [cons_bits, 65536) (test_tx_model_cpu.py holds that), so "the code word taken
    # without shorten()" is the same prefix and no wrong variant at all.  The variant "tail message bits not fixed" is the mistake
    # that does differ: those bits not fixed, here -1, and the code word's first cons_bits taken.
    mesg = np.full(m.mesg_bits, -1 if variant == "tail message bits not fixed" else 1, np.int8)
    mesg[:DATA_BITS] = 1 - 2 * np.unpackbits(inp, bitorder="little").astype(np.int8)  # encode.cc:293-294
    crc = int(L.orc_crc32_bytes(0xD419CC15, O.ptr(inp), O.DATA_BYTES))                # encode.cc:295-297
    mesg[DATA_BITS:CRC_BITS] = [1 - 2 * ((crc >> i) & 1) for i in range(32)]          # encode.cc:298-299
    fr = O.frozen(m.table)
    code = np.zeros(1 << 16, np.int8)
    L.orc_polar_sysenc(O.ptr(code), O.ptr(mesg), O.ptr(fr), 16)                       # encode.cc:302
    fz = _frozen_bits(m.table)
    k = np.cumsum(~fz) - 1                                                            # encode.cc:180-186: k before its increment
    keep = fz | (k < CRC_BITS)
    assert int(keep.sum()) == m.cons_bits
    out = (code[:m.cons_bits] if variant == "tail message bits not fixed" else code[keep]).astype(np.float64)
    if variant == "one code bit flipped":
        out[-1] = -out[-1]
    return out


def meta_bits(call_sign, mode):
    """encode.cc:155-173: the 255 NRZ values of the meta-data symbol before the differential step"""
    L = O.lib()
    cs = int(L.orc_base37_encode(call_sign.encode()))
    assert 0 < cs < 129961739795077                                                   # encode.cc:358
    md = (cs << 8) | mode                                                             # encode.cc:291
    bits = np.zeros(72, np.uint8)
    bits[:55] = [(md >> i) & 1 for i in range(55)]
    crc = int(L.orc_crc16_u64(0xA8F4, (md << 9) & O_M64))
    bits[55:71] = [(crc >> i) & 1 for i in range(16)]
    data = np.packbits(bits)                                                          # big-endian bits: CODE::set_be_bit
    parity = np.zeros(23, np.uint8)
    L.orc_bch_encode(O.ptr(data), O.ptr(parity))
    return 1.0 - 2.0 * np.concatenate([bits[:71], np.unpackbits(parity)[:MLS1_LEN - 71]]).astype(np.float64)


O_M64 = (1 << 64) - 1


def psk_map(b, mod_bits):
    """psk.hh:84-87 and 132-139 on NRZ rows [n, mod_bits]"""
    if mod_bits == 2:
        return math.sqrt(0.5) * (b[:, 0] + 1j * b[:, 1])
    c, s = math.cos(math.pi / 8), math.sin(math.pi / 8)
    re = np.where(b[:, 0] < 0, s, c)
    im = np.where(b[:, 0] < 0, c, s)
    return re * b[:, 1] + 1j * im * b[:, 2]


# ---------------------------------------------------------------- float stages
class _Encoder:
    def __init__(self, rate, mode, freq_off, variant):
        self.m, self.vr = MODES[mode], variant
        self.sl = symbol_len(rate)
        self.gl = self.sl // 8                                                        # encode.cc:32
        self.guard = np.zeros(self.gl, np.complex128)
        self.out = []
        offset = int(freq_off * self.sl / rate)                                       # encode.cc:283 (exact for multiples of 50)
        assert offset * rate == freq_off * self.sl
        if variant == "offset one bin off":
            offset += 1
        self.code_off = offset - self.m.cols // 2                                     # encode.cc:284
        self.mls0_off = offset - MLS0_LEN + 1                                         # encode.cc:285
        self.mls1_off = offset - MLS1_LEN // 2                                        # encode.cc:286
        self.fdom = np.zeros(self.sl, np.complex128)

    def improve_papr(self, temp):
        """encode.cc:80-100"""
        sl, n4 = self.sl, 4 * self.sl
        c = np.arange(-sl // 2, sl // 2)
        fdom4 = np.zeros(n4, np.complex128)
        fdom4[c % n4] = self.fdom[c % sl]
        tdom4 = np.fft.ifft(fdom4) * n4 / math.sqrt(n4)                               # bwd4, then / sqrt(4 symbol_len)
        amp = np.abs(tdom4) if self.vr == "clip by |v|" else np.maximum(np.abs(tdom4.real), np.abs(tdom4.imag))
        tdom4 = np.where(amp > 1.0, tdom4 / np.maximum(amp, 1.0), tdom4)
        fdom4 = np.fft.fft(tdom4)
        kept = (np.abs(temp[c % sl]) != 0) | (self.vr == "spill kept")
        temp[c % sl] = np.where(kept, fdom4[c % n4] / math.sqrt(n4), 0.0)
        return temp

    def symbol(self, papr=True):
        """encode.cc:101-131"""
        sl, gl = self.sl, self.gl
        temp = self.fdom.copy()
        if papr:
            temp = self.improve_papr(temp)
        tdom = np.fft.ifft(temp) * sl / math.sqrt(8 * sl)
        x = np.arange(gl) / (gl if self.vr == "ramp i/guard_len" else gl - 1)
        x = 0.5 * (1.0 - np.cos(math.pi * x))
        tail = tdom[:gl] if self.vr == "guard from the wrong end" else tdom[sl - gl:]
        self.out += [(1.0 - x) * self.guard + x * tail, tdom]                         # DSP::lerp; encode.cc:127-128
        self.guard = tdom[:gl].copy()

    def pilot_block(self):
        """encode.cc:132-141"""
        self.fdom[:] = 0
        i = np.arange(self.code_off, self.code_off + self.m.cols)
        self.fdom[i % self.sl] = math.sqrt(self.sl / self.m.cols) * mls_nrz(MLS2_POLY, self.m.cols)
        self.symbol()

    def schmidl_cox(self):
        """encode.cc:142-154: the differential step multiplies each carrier by the one before it, in ascending order"""
        self.fdom[:] = 0
        seq = np.cumprod(mls_nrz(MLS0_POLY, MLS0_LEN)) * math.sqrt(2 * self.sl / MLS0_LEN)
        self.fdom[(self.mls0_off - 2) % self.sl] = math.sqrt(2 * self.sl / MLS0_LEN)
        self.fdom[(2 * np.arange(MLS0_LEN) + self.mls0_off) % self.sl] = seq
        self.symbol(self.vr == "papr on schmidl-cox")

    def meta_data(self, nrz):
        """encode.cc:166-178"""
        self.fdom[:] = 0
        fac = math.sqrt(self.sl / MLS1_LEN)
        seq = np.cumprod(nrz) * fac
        if self.vr != "meta-data unscrambled":
            seq = seq * mls_nrz(MLS1_POLY, MLS1_LEN)
        self.fdom[(self.mls1_off - 1) % self.sl] = fac
        self.fdom[(np.arange(MLS1_LEN) + self.mls1_off) % self.sl] = seq
        self.symbol()

    def rows(self, code):
        """encode.cc:304-309: fdom keeps multiplying, row after row, from the pilot it still holds"""
        m = self.m
        idx = (np.arange(m.cols) + self.code_off) % self.sl
        pilot = self.fdom[idx].copy()
        pts = psk_map(code.reshape(-1, m.mod_bits), m.mod_bits).reshape(-1, m.cols)
        for j in range(pts.shape[0]):
            self.fdom[idx] = (pilot if self.vr == "rows multiply the pilot" else self.fdom[idx]) * pts[j]
            self.symbol(self.vr != "no papr on data rows")


def stream(payloads, mode, rate=8000, freq_off=0, call_sign="ANONYMOUS", channels=2, bits=16, variant=None):
    """the unrounded PCM of `encode OUT rate bits channels freq_off mode call_sign file..`, [samples, channels] float64 in LSB (8 bit:
    the offset of 128 included): rint of it is what an exact transmitter writes.  payloads: [count, 5380] unscrambled bytes."""
    assert variant is None or variant in VARIANTS, variant
    payloads = np.ascontiguousarray(payloads, np.uint8).reshape(-1, O.DATA_BYTES)
    e = _Encoder(rate, mode, freq_off, variant)
    nrz = meta_bits(call_sign, mode)
    e.pilot_block()                                                                   # encode.cc:288
    for k in range(payloads.shape[0]):
        if k and variant == "tail forgotten at a payload boundary":
            e.guard[:] = 0
        e.schmidl_cox()
        e.meta_data(nrz)
        e.pilot_block()
        e.rows(code_bits(payloads[k], mode, variant))
    e.fdom[:] = 0
    e.symbol()                                                                        # encode.cc:311-313
    lead = rate - 1 if variant == "rate - 1 leading silence" else rate                # encode.cc:423
    z = np.concatenate([np.zeros(lead, np.complex128)] + e.out + [np.zeros(2 * rate - lead, np.complex128)])   # encode.cc:441
    assert z.size == stream_samples(rate, mode, payloads.shape[0])
    if variant == "re and im swapped":
        z = z.imag + 1j * z.real
    x = np.stack([z.real, z.imag], axis=1)[:, :channels]                              # WritePCM::write(.., 2): one channel = re alone
    v = factor(bits) * np.clip(x, -1.0, 1.0)                                          # DSP::WriteWAV: clamp, scale, round
    if bits == 8:
        v = v + (127.0 if variant == "8-bit offset 127" else 128.0)
    return v


# ---------------------------------------------------------------- the case table (CPU: oracle against model; GPU: device against both)
Case = namedtuple("Case", "name rate mode channels bits freq_off count n_streams seed")
CALL_SIGN = "TX MODEL"


def cases():
    """A: every mode at 8 kHz, 2 channels, two one-payload streams, at a band edge (even modes the upper, odd modes the lower).  B: mono at 8 kHz,
    the lowest carrier at 0 Hz or the highest at Nyquist.  C: the other rates (the last one reaches +-32767).  D: several streams."""
    out = []
    for mode in range(6, 14):
        off = permitted_offsets(mode, 8000, 2)[-1 if mode % 2 == 0 else 0]
        out.append(Case("A mode %d" % mode, 8000, mode, 2, 16, off, 1, 2, 100 + mode))
    for mode, edge in ((6, 0), (9, -1), (10, 0), (13, -1)):
        out.append(Case("B mode %d mono" % mode, 8000, mode, 1, 16, permitted_offsets(mode, 8000, 1)[edge], 1, 1, 200 + mode))
    out += [Case("C 16 kHz mode 6 mono", 16000, 6, 1, 16, permitted_offsets(6, 16000, 1)[0], 1, 1, 301),
            Case("C 16 kHz mode 11 8 bit", 16000, 11, 2, 8, permitted_offsets(11, 16000, 2)[-1], 1, 1, 302),
            Case("C 44.1 kHz mode 10", 44100, 10, 2, 16, permitted_offsets(10, 44100, 2)[0], 1, 1, 303),
            Case("C 48 kHz mode 13 mono", 48000, 13, 1, 16, permitted_offsets(13, 48000, 1)[-1], 1, 1, 15),
            Case("D mode 12 count 3 x 2 streams", 8000, 12, 2, 16, 0, 3, 2, 401),
            Case("D mode 9 mono 8 bit count 2 x 3 streams", 8000, 9, 1, 8, 1400, 2, 3, 402),
            Case("D 48 kHz mode 10 count 2 x 2 streams", 48000, 10, 2, 16, -20450, 2, 2, 403)]
    return out


def case_payloads(case):
    """[n_streams, count, 5380]: every payload of a case distinct"""
    return np.stack([O.payload_for(1000 * case.seed + s, case.count).reshape(case.count, O.DATA_BYTES) for s in range(case.n_streams)])


def model_of(case, payloads, variant=None):
    return stream(payloads, case.mode, case.rate, case.freq_off, CALL_SIGN, case.channels, case.bits, variant)


def oracle_of(case, payloads):
    return O.encode_pcm(np.ascontiguousarray(payloads).reshape(-1), bits=case.bits, channels=case.channels, freq_off=case.freq_off,
                        call_sign=CALL_SIGN, mode=case.mode, rate=case.rate)
