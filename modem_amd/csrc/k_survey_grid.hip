// k_survey_grid.hip -- the grid survey: the mean output power of every slot of the grid front end's filter
// bank (section 4.19), as one row or as a waterfall of rows.  With D, M = 2 D, the taps h and y_k[n] of section 4.19 at ABSOLUTE
// output times n (x zero at negative positions) and S = times_per_row, a multiple of 8:
//   row r:  P[r][k + M / 2] = (1 / S) sum_{n = r S .. r S + S - 1} |y_k[n]|^2,   k = -M / 2 .. M / 2 - 1.
// k_survey_grid: one workgroup of 256 threads per tile of NT = max(8, 4096 / M) output times, the tiles counted from the call's first
// time row_first S - a multiple of 8, so a tile holds whole groups of 8 times (group g: the times 8 g .. 8 g + 7) and no group
// straddles a row.  Steps 1 and 2 are k_channelize_grid's: the same code, grid_bank.h's, so the same bytes in LDS:
//   1. the branch sums u_n[r] of the tile into LDS (time minor, rows of NT + 1), one FMA chain per component with a ascending;
//   2. the radix-2 decimation-in-frequency transform in place: natural order in, slot k's sum in row brev(k mod M) out;
//   3. every (LDS row, group of the tile) is reduced to one float and stored at part[(group counted from the call's first)][LDS row]:
//      lanes along the LDS rows, so the stores of a tile are one contiguous run, and the reads of 64 neighbouring rows stand
//      2 (NT + 1) dwords apart - an odd multiple of 2, so the 32 lanes of a half wave start on 32 different even banks of 64 and
//      their 8-byte reads cover every bank once (M >= 64; DESIGN.md 4.21 has the count for the small M).
// The sign (-1)^{k n} of section 4.19 drops out of a power and is not applied.
// k_survey_grid_rows: one thread per (row, LDS row) sums the row's S / 8 partials in ascending group order - the loads coalesced,
// up to 32 in flight and added in that order - multiplies by fp32(1 / S) and writes slot k = brev(LDS row) at its place k + M / 2
// of the row: the reversal and the shift are undone here, on 1 / S of the data.  k_survey_grid_rows_staged is the same sum for M <= 32
// and rows of 64 groups or more, one workgroup per row with the row's partials passed through LDS (see there): the same bytes.
// The order of the sum is part of the definition's contract and depends on absolute indices only: |y|^2 = fma(im, im, re re), one
// fp32 chain over the 8 times of a group in ascending time, one fp32 chain over a row's groups in ascending order, one product.
// No float atomics, no "last workgroup finishes".  All-zero input gives +0.
#include "dev_common.h"
#include "grid_bank.h"
#include "kernels.h"

namespace rx {

template <int FMT, int LOGM>
__global__ __launch_bounds__(GRID_THREADS) void k_survey_grid(SurveyGridArgs a)
{
	constexpr int M = 1 << LOGM, NT = grid_tile(LOGM), NTS = NT + 1, GRP = SURVEY_GRID_G;
	static_assert(grid_tile(LOGM) % SURVEY_GRID_G == 0, "a tile holds whole groups");
	__shared__ float2 u[M * NTS];
	const int tid = threadIdx.x;
	const long long j0 = (long long)blockIdx.x * NT;              // the tile's first time, counted from the call's first
	const long long n0 = a.t_first + j0;
	const int nt = (int)(a.n_times - j0 < NT ? a.n_times - j0 : NT);  // times of the tile that exist: a multiple of 8

	// ---- 1. the branch sums (a position below 0, or of a time past the tile's last that exists, lies outside the buffer: not loaded),
	// 2. the transform: slot k's sum in row brev(k mod M)
	grid_branch_sums<FMT, LOGM>(u, a, n0, tid);
	grid_dif<LOGM>(u, a.tw, tid);

	// ---- 3. the groups' powers: item (group g of the tile, LDS row), rows along the lanes; the tile's partials are one contiguous run
	float *dst = a.part + (size_t)(j0 / GRP) * M;
	for (int it = tid; it < (nt / GRP) * M; it += GRID_THREADS) {
		const int row = it & (M - 1), g = it >> LOGM;
		const float2 *x = u + row * NTS + g * GRP;
		float s = 0.f;
		#pragma unroll
		for (int t = 0; t < GRP; ++t) {
			const float2 v = x[t];
			s += __builtin_fmaf(v.y, v.y, v.x * v.x);
		}
		dst[it] = s;
	}
}

// row r_local, LDS row: the ordered chain over the row's groups, the loads in flight in batches and added in that order (as k_survey_rows)
__global__ __launch_bounds__(256) void k_survey_grid_rows(SurveyGridArgs a, float scale)
{
	const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
	const int M = 1 << a.logm;
	if (t >= a.n_rows * M)
		return;
	const long long r = t >> a.logm;
	const int row = (int)(t & (M - 1));
	const float *p = a.part + (size_t)r * (size_t)a.n_groups * M + row;
	// (a row of 4096 times is a chain of 512 loads per thread and a launch of few threads: 32 in flight while that many are left)
	float s = p[0];
	int g = 1;
	for (; g + 32 <= a.n_groups; g += 32) {
		float v[32];
		#pragma unroll
		for (int j = 0; j < 32; ++j)
			v[j] = p[(size_t)(g + j) * M];
		#pragma unroll
		for (int j = 0; j < 32; ++j)
			s += v[j];
	}
	for (; g + 8 <= a.n_groups; g += 8) {
		float v[8];
		#pragma unroll
		for (int j = 0; j < 8; ++j)
			v[j] = p[(size_t)(g + j) * M];
		#pragma unroll
		for (int j = 0; j < 8; ++j)
			s += v[j];
	}
	for (; g < a.n_groups; ++g)
		s += p[(size_t)g * M];
	const unsigned k = __brev((unsigned)row) >> (32 - a.logm);    // the slot mod M that stands in this LDS row
	a.out[r * M + (long long)(k ^ (unsigned)(M / 2))] = s * scale;   // k + M / 2 mod M: ascending slot order
}

// The same sum for M <= 32 and long rows: there a wave of k_survey_grid_rows holds 64 / M rows whose partials lie a whole row apart,
// so every load touches 64 / M lines for 4 M bytes each.  One workgroup per row instead: the row's partials - one contiguous run of
// n_groups M floats - pass through LDS in chunks of 4096 floats, loaded as float4 with every load of a chunk in flight, and thread
// `LDS row` < M adds its column of the chunk in ascending group order (stride M floats: M neighbouring banks).  The chain and its
// bytes are k_survey_grid_rows' (0 + p[0] = p[0]: the partials are no negative zeros).
constexpr int SVG_STAGE = 4096;
__global__ __launch_bounds__(256) void k_survey_grid_rows_staged(SurveyGridArgs a, float scale)
{
	__shared__ float4 buf4[SVG_STAGE / 4];
	const float *buf = (const float *)buf4;
	const int tid = threadIdx.x, M = 1 << a.logm;
	const long long r = blockIdx.x;
	const float4 *p = (const float4 *)(a.part + (size_t)r * (size_t)a.n_groups * M);   // (n_groups M is a multiple of 4: 16-byte aligned)
	const int per = SVG_STAGE >> a.logm;                          // groups per chunk
	float s = 0.f;
	for (int g0 = 0; g0 < a.n_groups; g0 += per) {
		const int ng = a.n_groups - g0 < per ? a.n_groups - g0 : per, n4 = (ng << a.logm) / 4;
		const float4 *q = p + ((size_t)g0 << a.logm) / 4;
		#pragma unroll 4
		for (int i = tid; i < n4; i += 256)
			buf4[i] = q[i];
		__syncthreads();
		if (tid < M) {
			int g = 0;
			for (; g + 8 <= ng; g += 8) {
				float v[8];
				#pragma unroll
				for (int j = 0; j < 8; ++j)
					v[j] = buf[((g + j) << a.logm) + tid];
				#pragma unroll
				for (int j = 0; j < 8; ++j)
					s += v[j];
			}
			for (; g < ng; ++g)
				s += buf[(g << a.logm) + tid];
		}
		__syncthreads();
	}
	if (tid < M) {
		const unsigned k = __brev((unsigned)tid) >> (32 - a.logm);
		a.out[r * M + (long long)(k ^ (unsigned)(M / 2))] = s * scale;
	}
}

template <int FMT> static void svg_launch(hipStream_t s, const SurveyGridArgs &a)
{
	grid_dispatch(a.logm, [&](auto c) {
		constexpr int LOGM = decltype(c)::value, NT = grid_tile(LOGM);
		hipLaunchKernelGGL((k_survey_grid<FMT, LOGM>), dim3((unsigned)((a.n_times + NT - 1) / NT)), dim3(GRID_THREADS), 0, s, a);
	});
}

void launch_survey_grid(hipStream_t s, const SurveyGridArgs &a, float scale)
{
	if (a.fmt == 0)
		svg_launch<0>(s, a);
	else if (a.fmt == 1)
		svg_launch<1>(s, a);
	else
		svg_launch<2>(s, a);
	if (a.logm <= 5 && a.n_groups >= 64)                          // (the same bytes either way)
		hipLaunchKernelGGL(k_survey_grid_rows_staged, dim3((unsigned)a.n_rows), dim3(256), 0, s, a, scale);
	else
		hipLaunchKernelGGL(k_survey_grid_rows, dim3((unsigned)(((a.n_rows << a.logm) + 255) / 256)), dim3(256), 0, s, a, scale);
}

}  // namespace rx
