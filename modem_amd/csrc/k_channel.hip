// k_channel.hip -- N3: build-owned channel models on the device (AWGN tile; multipath -> CFO -> SFO chain; Watterson fading).
#include "dev_common.h"
#include "kernels.h"

namespace rx {

// ---------------------------------------------------------------- channel model utility
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x)
{
	x += 0x9e3779b97f4a7c15ull;
	x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
	x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
	return x ^ (x >> 31);
}
// out frame f = base[f % n_base] + complex AWGN(sigma per component); counter-based RNG
__global__ __launch_bounds__(256) void k_awgn_tile(const short2 *__restrict__ base, size_t n_base, short2 *__restrict__ out,
	size_t spf, float sigma, unsigned long long seed, unsigned long long first_frame)
{
	const size_t f = blockIdx.x;
	const unsigned long long key = splitmix64(seed ^ splitmix64(first_frame + f + 0x1234567ull));
	const short2 *src = base + (f % n_base) * spf;
	short2 *dst = out + f * spf;
	for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < spf; i += (size_t)gridDim.y * 256) {
		unsigned long long r = splitmix64(key + i);
		float u1 = ((float)(unsigned)(r >> 40) + 0.5f) * (1.f / 16777216.f);
		float u2 = ((float)(unsigned)((r >> 8) & 0xffffff) + 0.5f) * (1.f / 16777216.f);
		float mag = sigma * sqrtf(-2.f * logf(u1));
		float sn, cs;
		sincosf(TWO_PI_F * u2, &sn, &cs);
		short2 v = src[i];
		float re = div_32767((float)v.x) + mag * cs, im = div_32767((float)v.y) + mag * sn;
		re = fminf(fmaxf(re, -1.f), 1.f);
		im = fminf(fmaxf(im, -1.f), 1.f);
		dst[i] = make_short2((short)nearbyintf(32767.f * re), (short)nearbyintf(32767.f * im));
	}
}

// grid = number of resident decoders (each needs 2 MiB of `soft`); 0 or >= n: one per codeword

void launch_awgn_tile(hipStream_t s, const int16_t *base, size_t n_base, int16_t *out, size_t n_out,
	size_t spf, float sigma, uint64_t seed, uint64_t first_frame)
{
	hipLaunchKernelGGL(k_awgn_tile, dim3((unsigned)n_out, 64), dim3(256), 0, s, (const short2 *)base, n_base, (short2 *)out,
		spf, sigma, (unsigned long long)seed, (unsigned long long)first_frame);
}

}  // namespace rx

// ---------------------------------------------------------------- build-owned channel chain (N3)
// README.md:49 pipes encode through aicodix/disorders: multipath | cfo | sfo | awgn.  That repository is
// absent; the definitions here are this build's own (same as oracle/channel.c, checked against it):
//   multipath: FIR with integer delays and complex gains;   cfo: x[m] * e^{j 2 pi hz m / rate};
//   sfo: out[i] = resample at t = i (1 + ppm 1e-6), 32-tap Hann-windowed sinc;   awgn: k_awgn_tile.
// 2-channel int16 in and out.  The chain is deterministic, so it is applied to the base frames once
// and k_awgn_tile then adds independent noise per frame.
namespace rx {

struct ChannelParams {
	float cfo_hz, sfo_ppm;
	int ntaps;
	int delays[8];
	float gre[8], gim[8];
};

__global__ __launch_bounds__(256) void k_channel(const short2 *__restrict__ in, short2 *__restrict__ out, size_t spf, ChannelParams cp, int rate)
{
	const size_t f = blockIdx.y;
	const short2 *src = in + f * spf;
	short2 *dst = out + f * spf;
	const double step = 1.0 + (double)cp.sfo_ppm * 1e-6;
	const double w0 = 2.0 * 3.14159265358979323846 * (double)cp.cfo_hz / (double)rate;
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < spf; i += (size_t)gridDim.x * 256) {
		auto stage12 = [&](long m) -> cf {   // multipath then cfo at integer sample m
			float re = 0.f, im = 0.f;
			for (int t = 0; t < cp.ntaps; ++t) {
				long idx = m - cp.delays[t];
				if (idx < 0 || (size_t)idx >= spf)
					continue;
				short2 v = src[idx];
				float xr = div_32767((float)v.x), xi = div_32767((float)v.y);
				re += xr * cp.gre[t] - xi * cp.gim[t];
				im += xr * cp.gim[t] + xi * cp.gre[t];
			}
			if (cp.cfo_hz != 0.f) {
				double a = w0 * (double)m;
				float c = (float)cos(a), s = (float)sin(a);
				float r2 = re * c - im * s, i2 = re * s + im * c;
				re = r2; im = i2;
			}
			return mk(re, im);
		};
		float ore, oim;
		if (cp.sfo_ppm == 0.f) {
			cf v = stage12((long)i);
			ore = v.re; oim = v.im;
		} else {
			const int HALF = 16;
			double t = (double)i * step;
			long t0 = (long)floor(t);
			double fr = t - (double)t0, re = 0.0, im = 0.0;
			for (int k = -HALF + 1; k <= HALF; ++k) {
				long idx = t0 + k;
				if (idx < 0 || (size_t)idx >= spf)
					continue;
				double x = (double)k - fr;
				double sinc = fabs(x) < 1e-12 ? 1.0 : sin(3.14159265358979323846 * x) / (3.14159265358979323846 * x);
				double w = 0.5 * (1.0 + cos(3.14159265358979323846 * x / (double)HALF));
				cf v = stage12(idx);
				re += sinc * w * v.re;
				im += sinc * w * v.im;
			}
			ore = (float)re; oim = (float)im;
		}
		ore = fminf(fmaxf(ore, -1.f), 1.f);
		oim = fminf(fmaxf(oim, -1.f), 1.f);
		dst[i] = make_short2((short)nearbyintf(32767.f * ore), (short)nearbyintf(32767.f * oim));
	}
}

void launch_channel(hipStream_t s, int rate, const int16_t *in, int16_t *out, size_t n, size_t spf, const void *params)
{
	ChannelParams cp = *(const ChannelParams *)params;
	hipLaunchKernelGGL(k_channel, dim3(128, (unsigned)n), dim3(256), 0, s, (const short2 *)in, (short2 *)out, spf, cp, rate);
}

}  // namespace rx

// ---------------------------------------------------------------- Watterson fading
// Every path's gain is a sum of FADING_SINES unit phasors whose frequencies are Gaussian (Hoeher), formed at knots FADING_KNOT
// samples apart and interpolated linearly between them; every quantity is a closed form of (seed, frame, sample index).
// One workgroup makes FADING_TILE samples of one frame: the frame's (increment, start phase) pairs, then the tile's knot gains
// into LDS (16 lanes per knot, one phasor each, summed by a butterfly so that the order of the sum is fixed), then one
// interpolated complex MAC per path and sample.  The delayed input is read through L2: the tile's own 16 KiB and its halo.
namespace rx {

constexpr int FADING_SINES = 16, FADING_KNOT = 32, FADING_TILE = 4096, FADING_KNOTS = FADING_TILE / FADING_KNOT + 1;

struct __attribute__((packed, aligned(4))) Short2x4 { unsigned a, b, c, d; };   // four I/Q pairs, I in the low half

struct FadingParams {
	int ntaps;
	int delays[8];
	float gre[8], gim[8], spread[8];
};

__global__ __launch_bounds__(256) void k_fading(const short2 *__restrict__ in, size_t n_in, short2 *__restrict__ out, size_t spf,
	FadingParams fp, int rate, unsigned long long seed, unsigned long long first_frame)
{
	__shared__ unsigned s_inc[8 * FADING_SINES], s_ph0[8 * FADING_SINES];
	__shared__ float2 s_gain[8][FADING_KNOTS];
	const size_t f = blockIdx.x;
	const size_t m0 = (size_t)blockIdx.y * FADING_TILE;
	const int tid = threadIdx.x;
	const int len = (int)min((size_t)FADING_TILE, spf - m0);      // the launch has no tile that starts at or past spf
	const int nk = ((len - 1) >> 5) + 2;                          // knots this tile reads: sample l uses l >> 5 and the next
	const unsigned long long key = splitmix64(seed ^ splitmix64(first_frame + f + 0x46414445ull));
	if (tid < FADING_SINES * fp.ntaps) {
		const int t = tid >> 4;
		const float spread = fp.spread[t];
		unsigned inc = 0, ph0 = 0;
		if (spread != 0.f) {                                      // (a specular path forms no sinusoids)
			const unsigned long long wf = splitmix64(key + 2ull * tid), wp = splitmix64(key + 2ull * tid + 1ull);
			const float u1 = ((float)(unsigned)(wf >> 40) + 0.5f) * (1.f / 16777216.f);
			const float u2 = ((float)(unsigned)((wf >> 8) & 0xffffff) + 0.5f) * (1.f / 16777216.f);
			const double z = sqrt(-2.0 * log((double)u1)) * cos(2.0 * 3.14159265358979323846 * (double)u2);
			const double f_hz = 0.5 * (double)spread * z;
			inc = (unsigned)(unsigned long long)llrint(f_hz * 4294967296.0 / (double)rate);
			ph0 = (unsigned)(wp >> 32);
		}
		s_inc[tid] = inc;
		s_ph0[tid] = ph0;
	}
	__syncthreads();
	// knot gains: item i = ((t * nk) + j) * 16 + k; its 16 lanes are neighbours of one wave and run every pass together
	const int items = fp.ntaps * nk * FADING_SINES;
	for (int base = 0; base < items; base += 256) {
		const int i = min(base + tid, items - 1);
		const int k = i & 15, tj = i >> 4, t = tj / nk, j = tj - t * nk;
		const unsigned phase = s_ph0[t * FADING_SINES + k] + s_inc[t * FADING_SINES + k] * ((unsigned)m0 + (unsigned)(FADING_KNOT * j));
		float sn, cs;
		phase_phasor(phase, cs, sn);
		#pragma unroll
		for (int m = 1; m < FADING_SINES; m <<= 1) {
			cs += __shfl_xor(cs, m);
			sn += __shfl_xor(sn, m);
		}
		if (k == 0 && base + tid < items) {
			const float gr = fp.gre[t], gi = fp.gim[t];
			const float cr = 0.25f * gr, ci = 0.25f * gi;         // 1 / sqrt(FADING_SINES), exact
			s_gain[t][j] = fp.spread[t] != 0.f ? make_float2(cr * cs - ci * sn, cr * sn + ci * cs) : make_float2(gr, gi);
		}
	}
	__syncthreads();
	const short2 *src = in + (f % n_in) * spf;
	short2 *dst = out + f * spf;
	// four consecutive samples per thread and pass: they lie between the same two knots, and each path's samples and the result
	// move as one 16-byte access (frames start on sample boundaries only, so the accesses are 4-byte aligned and no more).
	// WHOLE = 0: the tile's last one to three samples, when the frame does not end on a group.
	auto group = [&](int l, auto whole_c) {
		constexpr bool WHOLE = decltype(whole_c)::value != 0;
		const size_t m = m0 + l;
		const int j = l >> 5, r0 = l & (FADING_KNOT - 1);
		float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
		for (int t = 0; t < fp.ntaps; ++t) {
			const size_t d = (size_t)fp.delays[t];
			unsigned x[4] = {0u, 0u, 0u, 0u};
			if (WHOLE && m >= d) {
				const Short2x4 q = *(const Short2x4 *)(src + (m - d));
				x[0] = q.a; x[1] = q.b; x[2] = q.c; x[3] = q.d;
			} else {                                              // the frame's first samples and its last: x is zero outside the frame
				#pragma unroll
				for (int i = 0; i < 4; ++i)
					if ((WHOLE || l + i < len) && m + i >= d)
						x[i] = ((const unsigned *)src)[m + i - d];
			}
			const float2 g0 = s_gain[t][j], g1 = s_gain[t][j + 1];
			const float dr = g1.x - g0.x, di = g1.y - g0.y;
			#pragma unroll
			for (int i = 0; i < 4; ++i) {
				const float fr = (float)(r0 + i) * (1.f / FADING_KNOT);
				const float gr = g0.x + dr * fr, gi = g0.y + di * fr;
				const float xr = div_32767((float)(short)(x[i] & 0xffffu)), xi = div_32767((float)(short)(x[i] >> 16));
				re[i] += xr * gr - xi * gi;
				im[i] += xr * gi + xi * gr;
			}
		}
		unsigned y[4];
		#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const float a = fminf(fmaxf(re[i], -1.f), 1.f), b = fminf(fmaxf(im[i], -1.f), 1.f);
			y[i] = ((unsigned)(int)nearbyintf(32767.f * a) & 0xffffu) | ((unsigned)(int)nearbyintf(32767.f * b) << 16);
		}
		if (WHOLE) {
			Short2x4 q;
			q.a = y[0]; q.b = y[1]; q.c = y[2]; q.d = y[3];
			*(Short2x4 *)(dst + m) = q;
		} else {
			#pragma unroll
			for (int i = 0; i < 3; ++i)
				if (l + i < len)
					((unsigned *)dst)[m + i] = y[i];
		}
	};
	for (int l = tid * 4; l + 4 <= len; l += 1024)
		group(l, IntC<1>{});
	if ((len & 3) && tid == ((len >> 2) & 255))
		group(len & ~3, IntC<0>{});
}

size_t fading_tile_samples() { return FADING_TILE; }

void launch_fading(hipStream_t s, int rate, const int16_t *in, size_t n_in, int16_t *out, size_t n_out, size_t spf, const void *params,
	uint64_t seed, uint64_t first_frame)
{
	FadingParams fp = *(const FadingParams *)params;
	const size_t tiles = (spf + FADING_TILE - 1) / FADING_TILE;
	hipLaunchKernelGGL(k_fading, dim3((unsigned)n_out, (unsigned)tiles), dim3(256), 0, s, (const short2 *)in, n_in, (short2 *)out, spf, fp,
		rate, (unsigned long long)seed, (unsigned long long)first_frame);
}

}  // namespace rx
