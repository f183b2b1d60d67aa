// k_channelize_grid.hip -- the wideband front end on a channel grid: a polyphase filter bank.  Decimation
// D = 2, 4 .. 512, M = 2 D slots k = -M/2 .. M/2 - 1 with their centres at k rate / 2, the taps h of section 4.14 (T = 12 M + 1):
//   y_k[n] = sum_{t = 0 .. T - 1} h[t] x[n D - t] e^{-2 pi i k (n D - t) / M},   x zero outside the buffer,
// computed as
//   u_n[r] = sum_a h[r + M a] x[n D - r - M a],  r = 0 .. M - 1,  a = 0 .. 11 (and a = 12 for r = 0),
//   y_k[n] = (-1)^{k n} sum_r u_n[r] e^{+2 pi i k r / M}:  one pass of the filter for all slots, one inverse DFT of length M per
// output time, a sign.  No NCO: the only irrational numbers are the transform's roots, which the host makes in double (a.tw).
// One workgroup of 256 threads makes a tile of NT output times:
//   1. the branch sums of the tile into LDS, u[r][t] (time minor, rows of NT + 1).  The input is read from global memory, lanes along
//      r: 64 neighbouring sample frames per load.  Output times of one parity share their samples (n D and (n + 2) D lie M apart), so
//      a thread forms a run of 4 .. 16 such times of one branch from one pass over their samples in registers: 1.75 (D <= 64) to 4
//      (D = 512) loads per branch sum, not 12; what is left of the 24 times a sample enters meets it again in L1 / L2 (at D = 512
//      the span of a tile of 8 times is 134 KiB as fp32 - there is no room to stage it in LDS beside the tile);
//   2. the transform in place, decimation in frequency, radix 2, two stages per pass over LDS: natural order in, bit-reversed out.
//      Stage of half-length H: (p, q) = (x[i] + x[i + H], (x[i] - x[i + H]) w^{j M / (2 H)}), j = i mod H.  The order of every sum is
//      fixed by M alone, so an output does not depend on the tile, the launch or the block it belongs to;
//   3. the requested slots only: row brev(k mod M) of the tile, the sign, NT neighbouring outputs of one slot row per NT lanes - at
//      least 64 contiguous bytes per row.
// Contract on order: u_n[r] is one FMA chain per component, a ascending; a position outside [in_first, in_first + n_in) is never
// loaded and enters as +0.  No state: a capture cut into blocks, each with the T - 1 samples before it, gives the bytes of one call.
#include "dev_common.h"
#include "kernels.h"

namespace rx {

constexpr int CHG_THREADS = 256;
// output times per tile: 4096 points of LDS, and never fewer than 8 times (64 bytes of a slot row)
__host__ __device__ constexpr int chg_tile(int logm) { return (4096 >> logm) > 8 ? (4096 >> logm) : 8; }

__device__ __forceinline__ float2 chg_mul(float2 a, float2 w)
{
	return make_float2(__builtin_fmaf(a.x, w.x, -(a.y * w.y)), __builtin_fmaf(a.x, w.y, a.y * w.x));
}
// one butterfly of the stage whose root for this pair is w
__device__ __forceinline__ void chg_bfly(float2 &p, float2 &q, float2 w)
{
	const float2 s = make_float2(p.x + q.x, p.y + q.y), d = make_float2(p.x - q.x, p.y - q.y);
	p = s;
	q = chg_mul(d, w);
}

template <int FMT, int LOGM>
__global__ __launch_bounds__(CHG_THREADS) void k_channelize_grid(ChannelizeArgs a)
{
	constexpr int M = 1 << LOGM, D = M / 2, NT = chg_tile(LOGM), NTS = NT + 1, HIST = 12;
	__shared__ float2 u[M * NTS];
	const int tid = threadIdx.x;
	const long long j0 = (long long)blockIdx.x * NT;              // the tile's first output, counted from out_first
	const long long n0 = a.out_first + j0;
	const int nt = (int)(a.n_out - j0 < NT ? a.n_out - j0 : NT);  // output times of the tile that exist

	// ---- 1. the branch sums.  Times of one parity share their samples: with t = e + 2 s, sample a of time t is x[(n0 + e) D - r -
	// M (a - s)], so a thread takes a run of CH times of one parity of its branch r and loads the CH + 12 samples j = a - s = -(CH - 1)
	// .. 12 once each, newest first; sample j meets time s at tap a = j + s, and for a given s the taps still come in ascending a.
	// M < 256: 256 / M threads per branch, one run of 16 each; else the branches tid, tid + 256 .., both parities, runs of NT / 2
	{
		constexpr int G = M < CHG_THREADS ? CHG_THREADS / M : 1;      // threads per branch
		constexpr int CH = M < CHG_THREADS ? 16 : NT / 2;             // times per run (G CH = NT, or 2 CH = NT)
		static_assert((G > 1 ? G * CH : 2 * CH) == NT, "the runs tile the times");
		const int g = M < CHG_THREADS ? tid >> LOGM : 0;
		for (int r = tid & (M < CHG_THREADS ? M - 1 : CHG_THREADS - 1); r < M; r += CHG_THREADS) {
			float h[HIST + 1];
			#pragma unroll
			for (int i = 0; i < HIST; ++i)
				h[i] = a.taps[r + M * i];
			h[HIST] = r == 0 ? a.taps[M * HIST] : 0.f;
			for (int run = 0; run < (G > 1 ? 1 : 2); ++run) {
				const int e = G > 1 ? g & 1 : run, s0 = G > 1 ? (g >> 1) * CH : 0;
				const int tf = e + 2 * s0;                                // the run's first time: t = tf + 2 s
				float re[CH], im[CH];
				#pragma unroll
				for (int s = 0; s < CH; ++s)
					re[s] = im[s] = 0.f;
				const long long m0 = (n0 + tf) * D - r - a.in_first;      // sample j = 0 of the run, counted from the buffer's first
				#pragma unroll
				for (int j = -(CH - 1); j <= HIST; ++j) {
					if (j == HIST && r != 0)                                  // tap a = 12 exists for branch 0 alone
						continue;
					const long long m = m0 - (long long)M * j;
					float2 x = make_float2(0.f, 0.f);
					if (m >= 0 && m < a.n_in)
						x = iq_sample<FMT>(a.in, (size_t)m);
					#pragma unroll
					for (int s = 0; s < CH; ++s) {
						const int i = j + s;                                  // the tap
						if (i < 0 || i > HIST || (i == HIST && r != 0))
							continue;
						re[s] = __builtin_fmaf(h[i], x.x, re[s]);
						im[s] = __builtin_fmaf(h[i], x.y, im[s]);
					}
				}
				#pragma unroll
				for (int s = 0; s < CH; ++s)
					u[r * NTS + tf + 2 * s] = make_float2(re[s], im[s]);
			}
		}
	}
	__syncthreads();

	// ---- 2. the transform: the stages of half-length M / 2, M / 4 .. 1, two per pass (the last alone when their number is odd).
	// A pass takes the points i, i + Q, i + 2 Q, i + 3 Q (Q the second stage's half-length): stage 2 Q pairs (i, i + 2 Q) and
	// (i + Q, i + 3 Q), stage Q pairs (i, i + Q) and (i + 2 Q, i + 3 Q).  Work item (b, t): lanes along t where a tile has 64 times
	const float2 *tw = a.tw;
	#pragma unroll
	for (int lq = LOGM - 2; lq >= 0; lq -= 2) {
		const int Q = 1 << lq;
		for (int it = tid; it < (M / 4) * NT; it += CHG_THREADS) {
			int b, t;
			if (NT >= 64) {
				t = it & (NT - 1);
				b = it / NT;
			} else {
				b = it & (M / 4 - 1);
				t = it >> (LOGM - 2);
			}
			const int j = b & (Q - 1), i = ((b >> lq) << (lq + 2)) + j;
			float2 *x = u + i * NTS + t;
			float2 x0 = x[0], x1 = x[Q * NTS], x2 = x[2 * Q * NTS], x3 = x[3 * Q * NTS];
			// stage 2 Q: the roots w^{j' M / (4 Q)} of j' = j and j + Q; stage Q: w^{j M / (2 Q)} for both pairs
			const float2 wa = tw[j << (LOGM - 2 - lq)], wb = tw[(j + Q) << (LOGM - 2 - lq)], wc = tw[j << (LOGM - 1 - lq)];
			chg_bfly(x0, x2, wa);
			chg_bfly(x1, x3, wb);
			chg_bfly(x0, x1, wc);
			chg_bfly(x2, x3, wc);
			x[0] = x0;
			x[Q * NTS] = x1;
			x[2 * Q * NTS] = x2;
			x[3 * Q * NTS] = x3;
		}
		__syncthreads();
	}
	if (LOGM & 1) {                                               // the stage of half-length 1: its root is 1
		for (int it = tid; it < (M / 2) * NT; it += CHG_THREADS) {
			int b, t;
			if (NT >= 64) {
				t = it & (NT - 1);
				b = it / NT;
			} else {
				b = it & (M / 2 - 1);
				t = it >> (LOGM - 1);
			}
			float2 *x = u + 2 * b * NTS + t;
			float2 x0 = x[0], x1 = x[NTS];
			chg_bfly(x0, x1, tw[0]);
			x[0] = x0;
			x[NTS] = x1;
		}
		__syncthreads();
	}

	// ---- 3. the requested slots: slot k's sum stands in row brev(k mod M); (-1)^{k n}
	for (int it = tid; it < a.n_channels * NT; it += CHG_THREADS) {
		const int t = it & (NT - 1), c = it / NT;
		if (t >= nt)
			continue;
		const unsigned k = a.inc[c] >> (32 - LOGM);                   // inc = k 2^32 / M mod 2^32
		const unsigned row = __brev(k) >> (32 - LOGM);
		float2 v = u[row * NTS + t];
		if (k & (unsigned)(n0 + t) & 1u)
			v = make_float2(-v.x, -v.y);
		float2 *dst = a.dst ? (float2 *)(uintptr_t)a.dst[c] : (float2 *)a.out + (size_t)c * (size_t)a.out_stride;
		dst[j0 + t] = v;
	}
}

template <int FMT, int LOGM> static void chg_launch2(hipStream_t s, const ChannelizeArgs &a)
{
	constexpr int NT = chg_tile(LOGM);
	hipLaunchKernelGGL((k_channelize_grid<FMT, LOGM>), dim3((unsigned)((a.n_out + NT - 1) / NT)), dim3(CHG_THREADS), 0, s, a);
}

template <int FMT> static void chg_launch(hipStream_t s, const ChannelizeArgs &a)
{
	switch (a.p) {
	case 2: chg_launch2<FMT, 2>(s, a); break;
	case 4: chg_launch2<FMT, 3>(s, a); break;
	case 8: chg_launch2<FMT, 4>(s, a); break;
	case 16: chg_launch2<FMT, 5>(s, a); break;
	case 32: chg_launch2<FMT, 6>(s, a); break;
	case 64: chg_launch2<FMT, 7>(s, a); break;
	case 128: chg_launch2<FMT, 8>(s, a); break;
	case 256: chg_launch2<FMT, 9>(s, a); break;
	case 512: chg_launch2<FMT, 10>(s, a); break;
	}
}

// (the shortest tile is 8 output times: the grid's x stays below 2^31)
long long channelize_grid_max_outputs() { return 8LL * 0x7fffffffLL; }

void launch_channelize_grid(hipStream_t s, const ChannelizeArgs &a)
{
	if (a.fmt == 0)
		chg_launch<0>(s, a);
	else if (a.fmt == 1)
		chg_launch<1>(s, a);
	else
		chg_launch<2>(s, a);
}

}  // namespace rx
