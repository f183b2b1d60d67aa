// sync_accept.h -- what the batch scan (k_sync.hip) and the stream scan (k_stream.hip) share of the Schmidl-Cox search:
// P at one time by direct summation, and the accept part of a trigger (decode.cc:110-151) by one workgroup.
#pragma once
#include "dev_common.h"
#include "kernels.h"

// Decision-critical fp32 expressions (see k_sync.hip): no FMA contraction here, nor in the rest of a file that includes this
#pragma clang fp contract(off)

namespace rx {

// P at time t by direct summation (decode.cc:86), double accumulate
template <int RATE>
__device__ __forceinline__ void direct_P(const SampleSrc &src, long t, int lane, double &re, double &im)
{
	constexpr int BUFFER_LEN = RateCfg<RATE>::BUFFER_LEN, SEARCH_POS = RateCfg<RATE>::SEARCH_POS, HALF_LEN = RateCfg<RATE>::HS;
	double sr = 0.0, si = 0.0;
	long a0 = t - (BUFFER_LEN - 1 - (SEARCH_POS + HALF_LEN));   // newest u
	for (int q = 0; q < (HALF_LEN + 63) / 64; ++q) {
		if (q * 64 + lane >= HALF_LEN)
			break;
		long u = a0 - (q * 64 + lane);
		cf x = src.at(u), y = src.at(u + HALF_LEN);
		sr += (double)x.re * y.re + (double)x.im * y.im;
		si += (double)x.im * y.re - (double)x.re * y.im;
	}
	re = wave_sum_d(sr);
	im = wave_sum_d(si);
}
// decode.cc:110-151 for the trigger at sample g = base + BUFFER_LEN - 1, by a workgroup of 256 threads: derotate (frac_cfo, the
// window at base + symbol_pos + HALF_LEN; symbol_pos = SEARCH_POS - index_max), FFT, differential demod, FFT, x kern, IFFT,
// peak / runner-up (lane, wave: tid & 63, tid >> 6).  Returns accept (decode.cc:140-145) with the peak's bin (shift) and pos_err; the caller forms symbol_pos and
// cfo_rad from them (decode.cc:146-150).  buf / xr: HALF_LEN points of LDS each, rot: (HALF_LEN + 255) / 256, red_p / red_i: 4.
// The window's samples must be readable through src (mono input: its analytic signal formed beforehand).
template <int RATE>
__device__ __forceinline__ bool sc_accept_wg(cf *buf, cf *xr, cf *rot, float *red_p, int *red_i, const SampleSrc &src,
	const cf *tw, const cf *kern, long base, int symbol_pos, float frac_cfo, int tid, int lane, int wave, int &shift_out, int &pos_err_out)
{
	typedef RateCfg<RATE> RC;
	constexpr int HALF_LEN = RC::HS, GUARD_LEN = RC::GL, NT = 256;
	if (tid < (HALF_LEN + NT - 1) / NT)
		rot[tid] = phasor(frac_cfo, (long)NT * tid);
	const cf p_thread = phasor(frac_cfo, tid);
	__syncthreads();
	for (int i = tid; i < HALF_LEN; i += NT)                   // decode.cc:117-118
		buf[i] = cmul(src.at(base + i + symbol_pos + HALF_LEN), cmul(p_thread, rot[i / NT]));
	__syncthreads();
	fft_fwd<HALF_LEN, NT, RC::SL>(buf, tw, tid);
	for (int i = tid; i < HALF_LEN; i += NT)                   // decode.cc:120-121
		xr[i] = demod_or_erase(buf[i], buf[(i + HALF_LEN - 1) % HALF_LEN]);
	__syncthreads();
	fft_fwd<HALF_LEN, NT, RC::SL>(xr, tw, tid);
	// x kern, then backward transform as conj(FFT(conj(.)))
	for (int i = tid; i < HALF_LEN; i += NT)
		xr[i] = cconj(cmul(xr[i], kern[i]));
	__syncthreads();
	fft_fwd<HALF_LEN, NT, RC::SL>(xr, tw, tid);
	// decode.cc:127-139: peak = max, shift = first index of it, next = runner-up
	float pk = -1.f;
	int sh_i = 0x7fffffff;
	for (int i = tid; i < HALF_LEN; i += NT) {
		float p = cnorm(xr[i]);
		if (p > pk) { pk = p; sh_i = i; }
	}
	#pragma unroll
	for (int m = 32; m; m >>= 1) {
		float op = __shfl_xor(pk, m);
		int oi = __shfl_xor(sh_i, m);
		if (op > pk || (op == pk && oi < sh_i)) { pk = op; sh_i = oi; }
	}
	if (lane == 0) { red_p[wave] = pk; red_i[wave] = sh_i; }
	__syncthreads();
	pk = red_p[0]; sh_i = red_i[0];
	#pragma unroll
	for (int w = 1; w < 4; ++w)
		if (red_p[w] > pk || (red_p[w] == pk && red_i[w] < sh_i)) { pk = red_p[w]; sh_i = red_i[w]; }
	__syncthreads();
	float nx = 0.f;
	for (int i = tid; i < HALF_LEN; i += NT) {
		float p = cnorm(xr[i]);
		if (i != sh_i && p > nx) nx = p;
	}
	#pragma unroll
	for (int m = 32; m; m >>= 1)
		nx = fmaxf(nx, __shfl_xor(nx, m));
	if (lane == 0)
		red_p[wave] = nx;
	__syncthreads();
	nx = fmaxf(fmaxf(red_p[0], red_p[1]), fmaxf(red_p[2], red_p[3]));
	const float peak = fmaxf(pk, 0.f);
	const int shift = peak > 0.f ? sh_i : 0;
	bool accept = peak > nx * 4.f;                             // decode.cc:140-141
	int pos_err = 0;
	if (accept) {
		cf v = cconj(xr[shift]);
		pos_err = (int)nearbyintf(atan2f(v.im, v.re) * (float)HALF_LEN / TWO_PI_F);
		if (abs(pos_err) > GUARD_LEN / 2)                      // decode.cc:144-145
			accept = false;
	}
	shift_out = shift;
	pos_err_out = pos_err;
	return accept;
}

}  // namespace rx
