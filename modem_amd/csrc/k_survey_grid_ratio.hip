// k_survey_grid_ratio.hip -- the grid survey at any ratio P / Q: the mean output power of every slot of the
// ratio grid front end's filter bank (section 4.22), as one row or as a waterfall of rows.  With P / Q, M = 2 P, the taps h_q, the
// output times u_n = n P, i_n = u_n div Q, q_n = u_n mod Q, the slots k_first .. k_first + n_all - 1 (-P <= k Q < P) and y_k[n] of
// section 4.22 at ABSOLUTE output times n (x zero at negative positions), and S = times_per_row, a multiple of 8:
//   row r:  P[r][k - k_first] = (1 / S) sum_{n = r S .. r S + S - 1} |y_k[n]|^2.
// k_survey_grid_ratio: one workgroup of 256 threads per tile of NT output times (survey_grid_ratio_plan: a multiple of 8), the tiles
// counted from the call's first time row_first S - a multiple of 8, so a tile holds whole groups of 8 times (group g: the times
// 8 g .. 8 g + 7) and no group straddles a tile or a row.  Steps 1 and 2 are k_channelize_grid_ratio's: the same code,
// grid_ratio_bank.h's, so the same bytes in LDS:
//   1. the branch sums u_n[r] of the tile into LDS (time minor, rows of NT + 1), one FMA chain per component with a ascending;
//   2. the mixed-radix decimation-in-frequency transform in place: slot k's sum in the row of bin (-k Q) mod M, which inc[c] names
//      for slot index c = k - k_first (the front end's table entry; its upper half, the final rotation's exponent, is not used);
//   3. every (slot index c, group of the tile) is reduced to one float and stored at part[(group counted from the call's first)][c]:
//      lanes along c, so the stores of a tile are one contiguous run of (NT / 8) n_all floats - n_all per group, not M.
// The final rotation by the root of k Q i_n mod M has modulus 1, drops out of a power and is not applied.
// k_survey_grid_ratio_rows: one thread per (row, slot index) sums the row's S / 8 partials in ascending group order - the loads up to
// 32 in flight and added in that order - multiplies by fp32(1 / S) and writes out[r n_all + c]: the partials stand in slot order.
// The order of the sum is section 4.21's and depends on absolute indices only: |y|^2 = fma(im, im, re re), one fp32 chain over the 8
// times of a group in ascending time, one fp32 chain over a row's groups in ascending order, one product.  No float atomics, no
// "last workgroup finishes".  All-zero input gives +0.  The tile enters no output.
#include "dev_common.h"
#include "grid_bank.h"
#include "grid_ratio_bank.h"
#include "kernels.h"

namespace rx {

constexpr int SVR_LDS_PLAIN = 65536;   // a launch that asks for more dynamic LDS than this raises the kernel's limit first

template <int FMT, int CH>
__global__ __launch_bounds__(CGR_THREADS) void k_survey_grid_ratio(SurveyGridRatioArgs a, GridRatioPlan pl)
{
	extern __shared__ float2 svr_lds[];
	constexpr int GRP = SURVEY_GRID_G;
	const int M = pl.m, NT = pl.nt, NTS = NT + 1;
	cf *u = (cf *)svr_lds;                                        // [M][NTS]
	const int tid = threadIdx.x;
	const long long j0 = (long long)blockIdx.x * NT;              // the tile's first time, counted from the call's first
	const long long n0 = a.t_first + j0;
	const int nt = (int)(a.n_times - j0 < NT ? a.n_times - j0 : NT);  // times of the tile that exist: a multiple of 8

	// ---- 1. the branch sums (a position below 0, or of a time past the call's last, lies outside the buffer: not loaded),
	// 2. the transform: slot k's sum in the row of bin (-k Q) mod M
	cgr_branch_sums<FMT, CH>(u, a, M, NT, pl.n_taps, pl.groups, n0, tid);
	__syncthreads();
	cgr_transform(u, a.tw, pl.radices, tid, M, NT);

	// ---- 3. the groups' powers: item (group g of the tile, slot index c), slots along the lanes; the tile's partials are one run
	float *dst = a.part + (size_t)(j0 / GRP) * (size_t)a.n_all;
	for (int it = tid; it < (nt / GRP) * a.n_all; it += CGR_THREADS) {
		const int g = it / a.n_all, c = it - g * a.n_all;
		const cf *x = u + (a.inc[c] & 0xffffu) * NTS + g * GRP;
		float s = 0.f;
		#pragma unroll
		for (int t = 0; t < GRP; ++t) {
			const cf v = x[t];
			s += __builtin_fmaf(v.im, v.im, v.re * v.re);
		}
		dst[it] = s;
	}
}

// row r_local, slot index c: the ordered chain over the row's groups, the loads in flight in batches and added in that order (as
// k_survey_grid_rows)
__global__ __launch_bounds__(256) void k_survey_grid_ratio_rows(SurveyGridRatioArgs a, float scale)
{
	const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
	const int W = a.n_all;
	if (t >= a.n_rows * W)
		return;
	const long long r = t / W;
	const int c = (int)(t - r * W);
	const float *p = a.part + (size_t)r * (size_t)a.n_groups * W + c;
	float s = p[0];
	int g = 1;
	for (; g + 32 <= a.n_groups; g += 32) {
		float v[32];
		#pragma unroll
		for (int j = 0; j < 32; ++j)
			v[j] = p[(size_t)(g + j) * W];
		#pragma unroll
		for (int j = 0; j < 32; ++j)
			s += v[j];
	}
	for (; g + 8 <= a.n_groups; g += 8) {
		float v[8];
		#pragma unroll
		for (int j = 0; j < 8; ++j)
			v[j] = p[(size_t)(g + j) * W];
		#pragma unroll
		for (int j = 0; j < 8; ++j)
			s += v[j];
	}
	for (; g < a.n_groups; ++g)
		s += p[(size_t)g * W];
	a.out[t] = s * scale;                                         // out[r n_all + c]
}

// the front end's plan with the survey's tile: the plan's tile rounded down to a multiple of 8, and 8 where the plan's is 6 (P >= 432:
// up to 73 728 bytes of LDS - the tile has no i_n mod M array, the rotation being dropped); the runs of the branch sums follow the tile
GridRatioPlan survey_grid_ratio_plan(int p, int q)
{
	GridRatioPlan pl = channelize_grid_ratio_plan(p, q);
	const int nt = pl.nt & ~(SURVEY_GRID_G - 1);
	pl.nt = nt < SURVEY_GRID_G ? SURVEY_GRID_G : nt;
	channelize_grid_ratio_runs(pl, q);
	pl.lds = (size_t)pl.m * (size_t)(pl.nt + 1) * sizeof(float2);
	return pl;
}

template <int FMT, int CH> static hipError_t svr_launch2(hipStream_t s, const SurveyGridRatioArgs &a, const GridRatioPlan &pl)
{
	if (pl.lds > (size_t)SVR_LDS_PLAIN) {
		const hipError_t e = hipFuncSetAttribute((const void *)k_survey_grid_ratio<FMT, CH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
		if (e != hipSuccess)
			return e;
	}
	hipLaunchKernelGGL((k_survey_grid_ratio<FMT, CH>), dim3((unsigned)((a.n_times + pl.nt - 1) / pl.nt)), dim3(CGR_THREADS), pl.lds, s, a, pl);
	return hipSuccess;
}

template <int FMT> static hipError_t svr_launch(hipStream_t s, const SurveyGridRatioArgs &a)
{
	const GridRatioPlan pl = survey_grid_ratio_plan(a.p, a.q);
	switch (pl.ch) {
	case 1: return svr_launch2<FMT, 1>(s, a, pl);
	case 2: return svr_launch2<FMT, 2>(s, a, pl);
	case 4: return svr_launch2<FMT, 4>(s, a, pl);
	case 8: return svr_launch2<FMT, 8>(s, a, pl);
	default: return svr_launch2<FMT, 16>(s, a, pl);
	}
}

hipError_t launch_survey_grid_ratio(hipStream_t s, const SurveyGridRatioArgs &a, float scale)
{
	const hipError_t e = a.fmt == 0 ? svr_launch<0>(s, a) : a.fmt == 1 ? svr_launch<1>(s, a) : svr_launch<2>(s, a);
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(k_survey_grid_ratio_rows, dim3((unsigned)((a.n_rows * a.n_all + 255) / 256)), dim3(256), 0, s, a, scale);
	return hipSuccess;
}

}  // namespace rx
