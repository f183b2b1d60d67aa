// k_channelize_grid_ratio.hip -- the wideband front end on a channel grid at any ratio P / Q: section 4.19's
// polyphase filter bank with section 4.17's taps and output times and a mixed-radix transform.  P / Q in lowest terms, 1 <= Q <= 16,
// 2 Q <= P <= 512, P = 2^a 3^b 5^c; M = 2 P, T = 24 P div Q + 1, u_n = n P, i_n = u_n div Q, q_n = u_n mod Q; slot k (-P <= k Q < P)
// lies at k Q / M cycles per wideband sample:
//   y_k[n] = sum_{j = 0 .. T - 1} h_{q_n}[j] x[i_n - j] e^{-2 pi i (k Q (i_n - j) mod M) / M},   x zero outside the buffer,
// computed as
//   u_n[r] = sum_a h_{q_n}[r + M a] x[i_n - r - M a],  r = 0 .. M - 1,  over the a with r + M a <= T - 1,
//   y_k[n] = W^{-(k Q i_n mod M)} sum_r u_n[r] W^{+(k Q mod M) r},  W = e^{2 pi i / M}.
// The sum over r is bin b = (-k Q) mod M of the FORWARD transform X[b] = sum_r u[r] e^{-2 pi i b r / M}, which dev_common.h's
// Bfly<2 / 3 / 4 / 5> compute.  One workgroup of 256 threads makes a tile of NT output times (GridRatioPlan):
//   1. the branch sums of the tile into LDS, u[r][t] (time minor, rows of NT + 1), read from global memory with lanes along r.  The
//      times n and n + 2 Q share their tap phase and lie M samples apart, so a thread takes the run t = e + 2 Q s of one branch and
//      loads each of the run's samples once: section 4.19's reuse with stride 2 Q;
//   2. the transform in place, decimation in frequency, the plan's stages in turn: every 5, every 3, every 4, a last 2.  A stage of
//      radix R on blocks of N points, L = N / R: the points i, i + L .. i + (R - 1) L of a block (j = i mod L) go through Bfly<R>, and
//      output t = 1 .. R - 1 is multiplied by w^{j t M / N}, w = e^{-2 pi i / M} (not at L = 1, where the root is 1), and put back at
//      i + t L.  Natural order in, digit-reversed out: bin b of a block stands at (b mod R) L + [bin b div R of the sub-block].  The
//      order of every sum is fixed by M alone, so an output does not depend on the tile, the launch or the block it belongs to;
//   3. the requested slots only: the row of bin (-k Q) mod M, times the root w^{(k Q mod M)(i_n mod M) mod M} - one complex multiply -
//      NT neighbouring outputs of one slot row per NT lanes.
// Contract on order: u_n[r] is one FMA chain per component, a ascending; a position outside [in_first, in_first + n_in) is never
// loaded and enters as +0.  No state: a capture cut into blocks, each with the T - 1 samples before it, gives the bytes of one call.
#include "dev_common.h"
#include "grid_bank.h"
#include "kernels.h"

namespace rx {

constexpr int CGR_THREADS = 256;
constexpr int CGR_HIST = 13;           // taps per branch at most: T <= 12 M + 1
constexpr int CGR_LDS = 61440;         // bytes of a tile at most

// grid_bank.h's multiply on a cf
__device__ __forceinline__ cf cgr_mul(cf a, float2 w)
{
	const float2 v = grid_mul(make_float2(a.re, a.im), w);
	return mk(v.x, v.y);
}

// one stage of radix R on blocks of N points, every time of the tile
template <int R> __device__ __forceinline__ void cgr_stage(cf *u, const float2 *tw, int tid, int M, int N, int NT)
{
	const int NTS = NT + 1, L = N / R, step = M / N, nb = M / R;
	for (int it = tid; it < nb * NT; it += CGR_THREADS) {
		int b, t;
		if (NT >= 32) {                                               // lanes along t where a tile has that many times
			b = it / NT;
			t = it - b * NT;
		} else {
			t = it / nb;
			b = it - t * nb;
		}
		const int blk = b / L, j = b - blk * L;
		cf *x = u + (blk * N + j) * NTS + t;
		cf v[R];
		#pragma unroll
		for (int i = 0; i < R; ++i)
			v[i] = x[i * L * NTS];
		Bfly<R>::run(v);
		if (L > 1) {
			#pragma unroll
			for (int i = 1; i < R; ++i)
				v[i] = cgr_mul(v[i], tw[j * i * step]);
		}
		#pragma unroll
		for (int i = 0; i < R; ++i)
			x[i * L * NTS] = v[i];
	}
	__syncthreads();
}

template <int FMT, int CH>
__global__ __launch_bounds__(CGR_THREADS) void k_channelize_grid_ratio(ChannelizeArgs a, GridRatioPlan pl)
{
	extern __shared__ float2 cgr_lds[];
	const int M = pl.m, NT = pl.nt, NTS = NT + 1, T = pl.n_taps, Q = a.q, Q2 = 2 * a.q;
	cf *u = (cf *)cgr_lds;                                        // [M][NTS]
	int *imod = (int *)(cgr_lds + M * NTS);                       // [NT]: i_n mod M
	const int tid = threadIdx.x;
	const long long j0 = (long long)blockIdx.x * NT;              // the tile's first output, counted from out_first
	const long long n0 = a.out_first + j0;
	const int nt = (int)(a.n_out - j0 < NT ? a.n_out - j0 : NT);  // output times of the tile that exist

	if (tid < NT)
		imod[tid] = (int)(((n0 + tid) * a.p / Q) % M);

	// ---- 1. the branch sums.  Work item (r, e, g): branch r, the run of times t = tf + 2 Q s < NT, tf = e + 2 Q CH g (ns <= CH of
	// them).  Time s stands at i_tf + M s with the phase of tf, so sample a of time s is x[i_tf - r - M (a - s)]: the run loads the
	// samples j = a - s = -(ns - 1) .. na - 1 once each, newest first; sample j meets time s at tap a = j + s, and for a given s the taps
	// still come in ascending a.  (The plan picks CH so that a small M still gives every thread a run.)
	{
		const int E = Q2 < NT ? Q2 : NT;
		for (int w = tid; w < M * E * pl.groups; w += CGR_THREADS) {
			const int eg = w / M, r = w - eg * M, g = eg / E, e = eg - g * E;
			const int tf = e + Q2 * CH * g;                               // the run's first time
			if (tf >= NT)
				continue;
			const long long un = (n0 + tf) * a.p, i0 = un / Q;
			const int ph = (int)(un - i0 * Q);
			const int na = r < T ? (T - 1 - r) / M + 1 : 0;           // the taps r + M a <= T - 1 of the branch
			const int left = (NT - tf + Q2 - 1) / Q2, ns = left < CH ? left : CH;
			float h[CGR_HIST];
			#pragma unroll
			for (int i = 0; i < CGR_HIST; ++i)
				h[i] = i < na ? a.taps[(size_t)(r + M * i) * Q + ph] : 0.f;
			float re[CH], im[CH];
			#pragma unroll
			for (int s = 0; s < CH; ++s)
				re[s] = im[s] = 0.f;
			const long long m0 = i0 - r - a.in_first;                 // sample j = 0 of the run, counted from the buffer's first
			#pragma unroll
			for (int j = -(CH - 1); j < CGR_HIST; ++j) {
				if (j >= na || j + ns <= 0)
					continue;
				const long long m = m0 - (long long)M * j;
				float2 x = make_float2(0.f, 0.f);
				if (m >= 0 && m < a.n_in)
					x = iq_sample<FMT>(a.in, (size_t)m);
				#pragma unroll
				for (int s = 0; s < CH; ++s) {
					const int i = j + s;                                  // the tap
					if (i < 0 || i >= CGR_HIST)
						continue;
					if (i < na && s < ns) {
						re[s] = __builtin_fmaf(h[i], x.x, re[s]);
						im[s] = __builtin_fmaf(h[i], x.y, im[s]);
					}
				}
			}
			#pragma unroll
			for (int s = 0; s < CH; ++s)
				if (s < ns)
					u[r * NTS + tf + Q2 * s] = mk(re[s], im[s]);
		}
	}
	__syncthreads();

	// ---- 2. the transform: the plan's radices, four bits each, first stage lowest
	{
		int N = M;
		#pragma unroll
		for (int s = 0; s < 8; ++s) {
			const int R = (int)((pl.radices >> (4 * s)) & 15u);
			if (R == 0)
				break;
			switch (R) {
			case 5: cgr_stage<5>(u, a.tw, tid, M, N, NT); break;
			case 3: cgr_stage<3>(u, a.tw, tid, M, N, NT); break;
			case 4: cgr_stage<4>(u, a.tw, tid, M, N, NT); break;
			default: cgr_stage<2>(u, a.tw, tid, M, N, NT); break;
			}
			N /= R;
		}
	}

	// ---- 3. the requested slots: inc[c] = the row of bin (-k Q) mod M | (k Q mod M) << 16
	for (int it = tid; it < a.n_channels * NT; it += CGR_THREADS) {
		const int c = it / NT, t = it - c * NT;
		if (t >= nt)
			continue;
		const unsigned w = a.inc[c], row = w & 0xffffu, kq = w >> 16;
		const cf v = cgr_mul(u[row * NTS + t], a.tw[(kq * (unsigned)imod[t]) % (unsigned)M]);
		float2 *dst = a.dst ? (float2 *)(uintptr_t)a.dst[c] : (float2 *)a.out + (size_t)c * (size_t)a.out_stride;
		dst[j0 + t] = make_float2(v.re, v.im);
	}
}

// the plan of M = 2 P = 2^a 3^b 5^c: c stages of radix 5, b of radix 3, a div 2 of radix 4, a mod 2 of radix 2.  A tile holds 4096
// points and 8 .. 256 times where LDS allows it, an even number
GridRatioPlan channelize_grid_ratio_plan(int p, int q)
{
	GridRatioPlan pl{};
	pl.m = 2 * p;
	pl.n_taps = 24 * p / q + 1;
	int m = pl.m, s = 0;
	for (; m % 5 == 0; m /= 5)
		pl.radices |= 5u << (4 * s++);
	for (; m % 3 == 0; m /= 3)
		pl.radices |= 3u << (4 * s++);
	for (; m % 4 == 0; m /= 4)
		pl.radices |= 4u << (4 * s++);
	if (m == 2)
		pl.radices |= 2u << (4 * s++);
	int nt = 4096 / pl.m;
	nt = nt < 8 ? 8 : nt > 256 ? 256 : nt;
	const int fit = (CGR_LDS - 8 * pl.m) / (8 * pl.m + 4);
	nt = nt < fit ? nt : fit;
	nt &= ~1;                                                     // rows of NT + 1: an odd stride in LDS
	pl.nt = nt;
	// the run: as long as a residue has times and a branch has taps (a longer one saves no load; 16 at most), halved until the tile
	// has a run for every thread
	const int per = (nt + 2 * q - 1) / (2 * q), e = 2 * q < nt ? 2 * q : nt, na = (pl.n_taps + pl.m - 1) / pl.m;
	pl.ch = 1;
	while (pl.ch < per && pl.ch < 16 && pl.ch < na)
		pl.ch *= 2;
	while (pl.ch > 1 && pl.m * e * ((per + pl.ch - 1) / pl.ch) < CGR_THREADS)
		pl.ch /= 2;
	pl.groups = (per + pl.ch - 1) / pl.ch;
	pl.lds = (size_t)pl.m * (size_t)(nt + 1) * sizeof(float2) + (size_t)nt * sizeof(int);
	return pl;
}

// where bin b stands after the plan's stages
int channelize_grid_ratio_row(const GridRatioPlan &pl, int b)
{
	int n = pl.m, row = 0;
	for (int s = 0; s < 8; ++s) {
		const int r = (int)((pl.radices >> (4 * s)) & 15u);
		if (!r)
			break;
		n /= r;
		row += (b % r) * n;
		b /= r;
	}
	return row;
}

// (the shortest tile is 6 output times: the grid's x stays below 2^31)
long long channelize_grid_ratio_max_outputs() { return 6LL * 0x7fffffffLL; }

template <int FMT, int CH> static void cgr_launch2(hipStream_t s, const ChannelizeArgs &a, const GridRatioPlan &pl)
{
	hipLaunchKernelGGL((k_channelize_grid_ratio<FMT, CH>), dim3((unsigned)((a.n_out + pl.nt - 1) / pl.nt)), dim3(CGR_THREADS), pl.lds, s, a, pl);
}

template <int FMT> static void cgr_launch(hipStream_t s, const ChannelizeArgs &a)
{
	const GridRatioPlan pl = channelize_grid_ratio_plan(a.p, a.q);
	switch (pl.ch) {
	case 1: cgr_launch2<FMT, 1>(s, a, pl); break;
	case 2: cgr_launch2<FMT, 2>(s, a, pl); break;
	case 4: cgr_launch2<FMT, 4>(s, a, pl); break;
	case 8: cgr_launch2<FMT, 8>(s, a, pl); break;
	default: cgr_launch2<FMT, 16>(s, a, pl); break;
	}
}

void launch_channelize_grid_ratio(hipStream_t s, const ChannelizeArgs &a)
{
	if (a.fmt == 0)
		cgr_launch<0>(s, a);
	else if (a.fmt == 1)
		cgr_launch<1>(s, a);
	else
		cgr_launch<2>(s, a);
}

}  // namespace rx
