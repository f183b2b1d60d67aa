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
// Steps 1 and 2 stand in grid_ratio_bank.h, which the grid survey at a ratio (k_survey_grid_ratio.hip, section 4.24) shares.
#include "dev_common.h"
#include "grid_bank.h"
#include "grid_ratio_bank.h"
#include "kernels.h"

namespace rx {

constexpr int CGR_LDS = 61440;         // bytes of a tile at most

template <int FMT, int CH>
__global__ __launch_bounds__(CGR_THREADS) void k_channelize_grid_ratio(ChannelizeArgs a, GridRatioPlan pl)
{
	extern __shared__ float2 cgr_lds[];
	const int M = pl.m, NT = pl.nt, NTS = NT + 1, T = pl.n_taps, Q = a.q;
	cf *u = (cf *)cgr_lds;                                        // [M][NTS]
	int *imod = (int *)(cgr_lds + M * NTS);                       // [NT]: i_n mod M
	const int tid = threadIdx.x;
	const long long j0 = (long long)blockIdx.x * NT;              // the tile's first output, counted from out_first
	const long long n0 = a.out_first + j0;
	const int nt = (int)(a.n_out - j0 < NT ? a.n_out - j0 : NT);  // output times of the tile that exist

	if (tid < NT)
		imod[tid] = (int)(((n0 + tid) * a.p / Q) % M);

	// ---- 1. the branch sums, 2. the transform: grid_ratio_bank.h's
	cgr_branch_sums<FMT, CH>(u, a, M, NT, T, pl.groups, n0, tid);
	__syncthreads();
	cgr_transform(u, a.tw, pl.radices, tid, M, NT);

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

// the runs of the branch sums for the plan's tile: as long as a residue has times and a branch has taps (a longer one saves no load; 16
// at most), halved until the tile has a run for every thread
void channelize_grid_ratio_runs(GridRatioPlan &pl, int q)
{
	const int nt = pl.nt;
	const int per = (nt + 2 * q - 1) / (2 * q), e = 2 * q < nt ? 2 * q : nt, na = (pl.n_taps + pl.m - 1) / pl.m;
	pl.ch = 1;
	while (pl.ch < per && pl.ch < 16 && pl.ch < na)
		pl.ch *= 2;
	while (pl.ch > 1 && pl.m * e * ((per + pl.ch - 1) / pl.ch) < CGR_THREADS)
		pl.ch /= 2;
	pl.groups = (per + pl.ch - 1) / pl.ch;
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
	channelize_grid_ratio_runs(pl, q);
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
