"""float64 model of the wideband survey (k_survey.hip behind ofdmrx_util_survey, and the host-only band
finder ofdmrx_util_find_bands), and the tolerance the device is held to.

The definition.  Input: interleaved I/Q in S16, U8 or F32, scaled as oracle_lib.pcm_to_cf scales it (fp32); the buffer holds the
wideband positions in_first .. in_first + n_in - 1.  N in {1280, 2560, 5120}, H = N / 2; segment s >= 0 covers the positions s H ..
s H + N - 1.  Window: periodic Hann w[n] = 0.5 - 0.5 cos(2 pi n / N), computed in double, rounded once to fp32; U = sum w[n]^2 in
double over the fp32 values.  X_s[b] = sum_n w[n] x[s H + n] exp(-2 pi i b n / N).  Row r averages the S = segs_per_row segments
r S .. r S + S - 1; bin i = 0 .. N - 1 is the frequency (i - N / 2) Rw / N:
    P[r][i] = (1 / (S U)) sum_s |X_s[(i + N / 2) mod N]|^2
White noise of power sigma^2 per complex sample reads sigma^2 in every bin.  The model evaluates this in float64 on the fp32 window
and the fp32-scaled input.

Summation order of the device (part of the contract, fixed by absolute indices only): |X|^2 = fma(im, im, re re); one fp32 chain
over the segments of a group of G = 8 consecutive segments counted from the row's first; then one fp32 chain over the groups in
ascending order; one product with fp32(1 / (S U)).

The tolerance, per bin of a row, derived here and from nothing the device gives.  u = 2^-24 (half an ulp, relative), K = the
number of radix stages of the transform (1280 = 5.4.4.4.4: 5; 2560 = 5.4.4.4.4.2 and 5120 = 5.4^5: 6), E_s = sum_n |w[n] x[s H +
n]|^2 the windowed segment's energy, so that sum_b |X_s[b]|^2 = N E_s (Parseval).
  * the window product: each component is rounded once, |delta_n| <= u |w[n] x[n]|; on any bin that is at most sum_n |delta_n| <=
    u sqrt(N) sqrt(E_s) (Cauchy-Schwarz);
  * a radix stage is sqrt(R) times a unitary map, so an error made in one stage reaches the output with the growth the signal
    itself has, and the 2-norm of the output's error is at most the sum over the stages of (relative error of a stage) sqrt(N E_s).
    A stage: the twiddle (its table entry rounded from double, u; a complex product, < 3 u) 4 u; the butterfly - radix 4: two levels
    of additions of values bounded by sum_t |v_t| <= 2 |v|, four outputs, 8 u |v| against an output norm of 2 |v|: 4 u; radix 5:
    five roundings per component on values bounded by sum_t |v_t| <= sqrt 5 |v|, five outputs: 25 u |v| against sqrt 5 |v|: < 12 u.
    Together at most 16 u per stage.  The error of one bin is at most the 2-norm of the whole error.
  So the amplitude of bin b of segment s is off by at most e_s = u (1 + 16 K) sqrt(N E_s), and |X|^2 by at most 2 |X| e_s + e_s^2.
  * |X|^2 in fp32 (a product and a fused multiply-add), the chain over the group (at most G - 1 additions), the chain over the n_g =
    ceil(S / G) groups (n_g - 1), the scale (rounded from double, and the product): every term is positive, so each rounding is at
    most u times the final sum: (G + n_g + 4) u of the row's value.
      tol[r][i] = (1 / (S U)) sum_s (2 |X_s| e_s + e_s^2) + (G + n_g + 4) u (P[r][i] + that)
The bound is homogeneous (degree 2) in x, so F32 input of any scale needs nothing added.  It is a worst-case bound: roundings do
not all point one way, and an fp32 evaluation stays at a few per cent of it (test_survey_model_cpu.py holds it to a quarter).

The band finder, on ONE row, in float64: floor = max(median of the N values, abs_floor), the median the mean of the two middle
values; bin i occupied when P[i] > floor 10^(thr_db / 10) and P[i] > 0; occupied bins separated by at most floor(gap_hz / (Rw / N))
unoccupied bins form one run (no wrap round the band edge); a run first .. last has width (last - first + 1) Rw / N and is kept when
that is >= min_width_hz; centre = ((first + last) / 2 - N / 2) Rw / N; power = mean of P over first .. last; level_db = 10 log10(power
/ floor).  The median is the noise floor only while less than half the band is occupied."""
import numpy as np

import channelize_model as CM

NFFT = (1280, 2560, 5120)
G = 8
U24 = 2.0 ** -24


def radices(N):
    """the plan of dev_common.h FftPlan: all 5s, then 7s, 3s, 4s and a final 2"""
    out, rem = [], N
    while rem > 1:
        R = 5 if rem % 5 == 0 else 7 if rem % 7 == 0 else 3 if rem % 3 == 0 else 4 if rem % 4 == 0 else 2
        out.append(R)
        rem //= R
    return out


def window64(N, kind="hann"):
    n = np.arange(N, dtype=np.float64)
    if kind == "hann":
        return 0.5 - 0.5 * np.cos(2 * np.pi * n / N)
    if kind == "symmetric":
        return 0.5 - 0.5 * np.cos(2 * np.pi * n / (N - 1))
    if kind == "hamming":
        return 0.54 - 0.46 * np.cos(2 * np.pi * n / N)
    return np.ones(N)                                               # rectangular


def window(N):
    """the fp32 window of the definition"""
    return window64(N).astype(np.float32)


def n_segments(W, N):
    """whole segments in positions 0 .. W - 1"""
    return max((W - N // 2) // (N // 2), 0)


def _segments(x, in_first, N, hop, first, count):
    """x holds positions in_first .. -> [count, N] rows x[s hop .. s hop + N - 1], s = first .."""
    lo, hi = first * hop, (first + count - 1) * hop + N
    assert count > 0 and lo >= in_first and hi <= in_first + len(x), "a position the rows need is not in the buffer"
    v = np.lib.stride_tricks.sliding_window_view(x[lo - in_first:hi - in_first], N)[::hop]
    assert v.shape[0] == count
    return v


def psd(pcm, nfft, segs_per_row=None, row_first=0, n_rows=None, in_first=0, variant=None):
    """-> (P [n_rows, nfft] float64, tol [n_rows, nfft]).  pcm: [W, 2] int16 / uint8 / float32, the wideband positions in_first ..;
    segs_per_row None: one row over everything; variant: one of VARIANTS, a deliberately wrong model"""
    N, H = nfft, nfft // 2
    pcm = np.ascontiguousarray(pcm)
    if variant == "u8 without offset" and pcm.dtype == np.uint8:
        x = pcm.astype(np.float32).astype(np.float64) / 127.0
        x = x[:, 0] + 1j * x[:, 1]
    else:
        x = CM.to_cf(pcm)
    if variant == "re / im swapped":
        x = x.imag + 1j * x.real
    total = n_segments(in_first + len(x), N)
    S = total if segs_per_row is None else segs_per_row
    if n_rows is None:
        n_rows = 1 if segs_per_row is None else total // S - row_first
    kind = {"rectangular": "rect", "hamming": "hamming", "symmetric hann": "symmetric"}.get(variant, "hann")
    w = window64(N, kind).astype(np.float32).astype(np.float64)
    if variant == "window squared":
        w = w * w
    w_true = window(N).astype(np.float64)
    U = 1.0 if variant == "U missing" else float((w_true * w_true).sum())
    hop = N if variant == "hop N" else H
    K = len(radices(N))
    n_g = -(-S // G)
    P = np.zeros((n_rows, N))
    tol = np.zeros((n_rows, N))
    for j in range(n_rows):
        r = row_first + j
        s0 = r * S + (1 if variant == "row starts one late" else 0)
        seg = _segments(x, in_first, N, hop, s0, S)
        X = np.fft.fft(seg * w, axis=1)
        p = (np.abs(X) ** 2).sum(axis=0) / (U if variant == "1 / S missing" else S * U)
        shift = N // 2 + (1 if variant == "shift off by one" else 0)
        P[j] = np.roll(p, shift)
        # the tolerance always from the definition
        segt = _segments(x, in_first, N, H, r * S, S) * w_true if variant else seg * w
        Xt = np.fft.fft(segt, axis=1) if variant else X
        e = U24 * (1 + 16 * K) * np.sqrt(N * (np.abs(segt) ** 2).sum(axis=1))
        amp = (2.0 * np.abs(Xt) * e[:, None] + (e * e)[:, None]).sum(axis=0) / (S * float((w_true * w_true).sum()))
        pt = (np.abs(Xt) ** 2).sum(axis=0) / (S * float((w_true * w_true).sum()))
        tol[j] = np.roll(amp + (G + n_g + 4) * U24 * (pt + amp), N // 2)
    return P, tol


VARIANTS = ("hop N", "rectangular", "hamming", "symmetric hann", "U missing", "1 / S missing", "re / im swapped", "shift off by one",
            "row starts one late", "u8 without offset", "window squared")


def fft_fp32(buf):
    """the Stockham plan of dev_common.h on [.., N] complex64, every product and sum in fp32 (the butterflies as plain DFT sums)"""
    N = buf.shape[-1]
    tw = np.exp(-2j * np.pi * np.arange(N) / N).astype(np.complex64)
    P = 1
    for R in radices(N):
        T = N // R
        b = np.arange(T)
        k = b % P
        v = [buf[..., b + t * T] for t in range(R)]
        if P > 1:
            v = [v[0]] + [(v[t] * tw[(t * k) * (N // (P * R))]).astype(np.complex64) for t in range(1, R)]
        wr = np.exp(-2j * np.pi * np.arange(R) / R).astype(np.complex64)
        new = np.empty_like(buf)
        j = (b - k) * R + k
        for q in range(R):
            y = v[0].copy()
            for t in range(1, R):
                y = (y + v[t] * wr[(q * t) % R]).astype(np.complex64)
            new[..., j + q * P] = y
        buf = new
        P *= R
    return buf


def psd_fp32(pcm, nfft, segs_per_row, row_first=0, n_rows=1):
    """an fp32 numpy evaluation in the kernel's order -> [n_rows, nfft] float32 (positions from 0)"""
    import oracle_lib as O
    f32 = np.float32
    N, H, S = nfft, nfft // 2, segs_per_row
    xc = O.pcm_to_cf(np.ascontiguousarray(pcm)).astype(f32)
    w = window(N)
    U = float((w.astype(np.float64) ** 2).sum())
    scale = f32(1.0 / (S * U))
    out = np.zeros((n_rows, N), f32)
    for j in range(n_rows):
        s0 = (row_first + j) * S
        total = None
        for g0 in range(0, S, G):
            acc = np.zeros(N, f32)
            for s in range(s0 + g0, s0 + min(g0 + G, S)):
                seg = xc[s * H:s * H + N]
                buf = ((w * seg[:, 0]).astype(f32) + 1j * (w * seg[:, 1]).astype(f32)).astype(np.complex64)
                X = fft_fp32(buf)
                acc = (acc + ((X.real * X.real).astype(f32) + (X.imag * X.imag).astype(f32)).astype(f32)).astype(f32)
            total = acc if total is None else (total + acc).astype(f32)
        out[j] = np.roll((total * scale).astype(f32), N // 2)
    return out


def worst(got, P, tol):
    """largest |got - P| / tol"""
    d = np.abs(np.asarray(got, np.float64) - P)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, d / np.where(tol > 0, tol, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def find_bands(row, rate_wide, thr_db=6.0, gap_hz=200.0, min_width_hz=1000.0, abs_floor=0.0):
    """-> (list of dicts in ascending frequency, floor); float64 on the row's values as given"""
    p = np.asarray(row).astype(np.float64)
    N = len(p)
    v = np.sort(p)
    floor = max(0.5 * (v[N // 2 - 1] + v[N // 2]), abs_floor)
    level = floor * 10.0 ** (thr_db / 10.0)
    bin_hz = rate_wide / N
    gap_bins = np.floor(gap_hz / bin_hz)
    occ = np.flatnonzero((p > level) & (p > 0.0))
    runs = []
    for i in occ:
        if runs and i - runs[-1][1] - 1 <= gap_bins:
            runs[-1][1] = int(i)
        else:
            runs.append([int(i), int(i)])
    out = []
    for first, last in runs:
        width = (last - first + 1) * bin_hz
        if not width >= min_width_hz:
            continue
        power = float(p[first:last + 1].sum()) / (last - first + 1)
        with np.errstate(divide="ignore"):
            level_db = float(np.float32(10.0 * np.log10(np.float64(power) / np.float64(floor))))
        out.append({"centre_hz": (0.5 * (first + last) - N // 2) * bin_hz, "width_hz": width, "power": power, "level_db": level_db,
                    "first_bin": first, "last_bin": last})
    return out, floor
