// api_streams.cpp -- the stream entries: ofdmrx_decode_streams*, many recordings in one call, and
// ofdmrx_decode_stream*, every preamble of one recording in one call: a batch of one recording, at the end of this file.
//   the stream scan (k_stream.hip, the SourceBatch forms) with the recording as a second grid dimension: [mono: the DC blocker's kept
//   states by a scan over tiles, the analytic signal of every recording] | the timing metric and the trigger as a scan over tiles |
//   decode.cc:110-151 for every falling edge - every recording from its own position 0, with its own tile count, nothing carried
//   from one into the next
//   | records: the SyncState of every accepted preamble, as a SKIP round with skip_left = 0 leaves it, at its place in the packed
//   order, with the recording it reads
//   one read-back of all recordings' edge / preamble counts (the call's host synchronisation)
//   the packed records through the chunk pipeline of the batch entries (api_pipeline.cpp: decode_records): a chunk takes whichever
//   recordings its records belong to
#include "api_internal.h"

namespace {

struct StreamsCall {                                              // what the checks leave: the lengths as the kernels take them
	size_t n_streams = 0;
	long max_len = 0;
	long long total_tiles = 0;
};

// every OFDMRX_E_ARG of the entries but the open feed; fills the handle's host arrays only when everything holds (so a call that
// fails here has touched nothing, the handle included)
int streams_args(ofdmrx_handle *h, const void *samples, int fmt, int channels, size_t n_streams, size_t stride, const size_t *n_samples,
	size_t max_records, const void *payload, const void *results, const size_t *n_preambles, const size_t *first_record, StreamsCall *call)
{
	if (!h || !samples || !n_samples || !n_preambles || !first_record || n_streams < 1 || n_streams > 65535)
		return OFDMRX_E_ARG;
	if (max_records && (!payload || !results))
		return OFDMRX_E_ARG;
	if (int r = check_samples(samples, fmt, channels))
		return r;
	const size_t frame_bytes = sample_bytes(fmt) * (size_t)channels;
	size_t longest = 0;
	for (size_t s = 0; s < n_streams; ++s) {
		if (n_samples[s] > (size_t)0x7fffffff / 2)
			return OFDMRX_E_ARG;
		longest = std::max(longest, n_samples[s]);
	}
	if (stride % frame_bytes || stride < longest * frame_bytes)
		return OFDMRX_E_ARG;
	call->n_streams = n_streams;
	call->max_len = (long)longest;
	return 0;
}

// the lengths and what follows from them, on the host (kept in the handle: the uploads read them) and on the device
int upload_lengths(ofdmrx_handle *h, const size_t *n, const size_t *given_n, StreamsCall *call)
{
	const size_t S = call->n_streams;
	h->sxs_len_h.resize(S);
	h->sxs_tile0_h.resize(S + 1);
	h->sxs_given0_h.resize(S);
	long long tiles = 0, at = 0;
	for (size_t s = 0; s < S; ++s) {
		h->sxs_len_h[s] = (int)n[s];
		h->sxs_tile0_h[s] = tiles;
		tiles += (long long)((n[s] + STREAM_TILE - 1) / STREAM_TILE);
		h->sxs_given0_h[s] = at;
		at += given_n ? (long long)given_n[s] : 0;
	}
	h->sxs_tile0_h[S] = tiles;
	call->total_tiles = tiles;
	int r = h->sxs_len.ensure(S * sizeof(int));
	r = r ? r : h->sxs_tile0.ensure((S + 1) * sizeof(long long));
	r = r ? r : h->sxs_given0.ensure(S * sizeof(long long));
	r = r ? r : h->sx_counts.ensure(std::max<size_t>(2, 2 * S) * sizeof(long long));
	if (r)
		return r;
	hipStream_t s = h->stream;
	HIP_OK(hipMemcpyAsync(h->sxs_len.p, h->sxs_len_h.data(), S * sizeof(int), hipMemcpyHostToDevice, s));
	HIP_OK(hipMemcpyAsync(h->sxs_tile0.p, h->sxs_tile0_h.data(), (S + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
	if (given_n)
		HIP_OK(hipMemcpyAsync(h->sxs_given0.p, h->sxs_given0_h.data(), S * sizeof(long long), hipMemcpyHostToDevice, s));
	return 0;
}

SourceBatch source_batch(const ofdmrx_handle *h, FrameBatch fb)
{
	return SourceBatch{ fb, nullptr, h->sxs_len.as<int>(), h->sxs_tile0.as<long long>(), h->sxs_given0.as<long long>() };
}

// The scan of all recordings of fb (device memory, fb.frame_stride_bytes apart, fb.samples_per_frame = the longest) and the packed
// records through the pipeline.  n_pre[s]: accepted preambles; first[s]: the uncapped packing (n_streams + 1).
// *n_written: records written, min(first[n_streams], max_records)
int decode_streams_dev(ofdmrx_handle *h, FrameBatch fb, const StreamsCall &call, size_t max_per_stream, size_t max_records, Outputs out,
	size_t *n_pre, size_t *first, size_t *n_written)
{
	hipStream_t s = h->stream;
	const size_t S = call.n_streams;
	const long max_len = call.max_len;
	*n_written = 0;
	h->last_n = 0;
	h->last_first = 0;
	if (max_len == 0) {                                           // nothing but empty recordings
		std::fill(n_pre, n_pre + S, (size_t)0);
		std::fill(first, first + S + 1, (size_t)0);
		HIP_OK(hipStreamSynchronize(s));
		return finish_call(h, 0);
	}
	int r = ensure_events(h, 16);
	if (r)
		return r;
	// Every recording's share of the edge buffer: a preamble every frame and a few noise triggers fit in max(4096, n / 2048), while all
	// shares together stay within 64 MiB (S <= 512), then less, down to 256 edges (S = 65535: 0.5 GiB).  A share that proved too small
	// has been grown (below) and stays grown for the handle's later calls.
	const long share0 = std::max(256L, std::min(4096L, (long)((64u << 20) / sizeof(StreamEdge) / S)));
	h->sxs_edge_cap = std::max(h->sxs_edge_cap, std::max(share0, max_len / 2048));
	const size_t e0 = mark(h, s);
	FrameBatch fb2 = fb;                                          // what the scan and the pipeline read: I/Q pairs
	if (fb.channels == 1) {                                       // D1 over every recording, then their analytic signals read as I/Q pairs
		const int ck_per = mono_ck_per_frame(max_len);
		r = h->sx_dc_end.ensure((size_t)call.total_tiles * sizeof(double));
		r = r ? r : h->sx_dc_in.ensure((size_t)call.total_tiles * sizeof(double));
		r = r ? r : h->sx_ck.ensure(S * (size_t)ck_per * sizeof(double));
		r = r ? r : h->sx_z.ensure(S * (size_t)max_len * sizeof(cf));
		if (r)
			return r;
		Range rg("ofdmrx:streams_front");
		const SourceBatch sb = source_batch(h, fb);
		launch_streams_dc(s, (int)S, max_len, sb, h->host.front, h->sx_dc_end.as<double>(), h->sx_dc_in.as<double>(), h->sx_ck.as<double>(), ck_per);
		launch_streams_front(s, h->rate, (int)S, max_len, sb, mono_args(h->host.front, h->sx_ck.as<double>(), ck_per), h->sx_z.as<cf>());
		fb2 = FrameBatch{ h->sx_z.p, (size_t)max_len * sizeof(cf), max_len, OFDMRX_FMT_F32, 2 };
	}
	const size_t e1 = mark(h, s);
	const SourceBatch sb2 = source_batch(h, fb2);
	std::vector<long long> &counts = h->sxs_counts_h;
	counts.assign(2 * S, 0);
	for (int pass = 0; pass < 2; ++pass) {
		const long cap = h->sxs_edge_cap;
		const size_t per = std::min<size_t>(max_per_stream, (size_t)cap);
		const size_t max_rec = std::min(max_records, S * per);
		r = h->sx_fn.ensure((size_t)call.total_tiles * sizeof(StreamFn));
		r = r ? r : h->sx_carry.ensure((size_t)call.total_tiles * sizeof(StreamCarry));
		r = r ? r : h->sx_edges.ensure(S * (size_t)cap * sizeof(StreamEdge));
		r = r ? r : h->sx_rec.ensure(std::max<size_t>(1, max_rec) * sizeof(SyncState));
		r = r ? r : h->sxs_rec_src.ensure(std::max<size_t>(1, max_rec) * sizeof(int));
		r = r ? r : h->sxs_first.ensure((S + 1) * sizeof(long long));
		if (r)
			return r;
		{
			Range rg("ofdmrx:streams_scan");
			HIP_OK(hipMemsetAsync(h->sx_counts.p, 0, 2 * S * sizeof(long long), s));
			launch_streams_scan(s, h->rate, (int)S, max_len, sb2, nullptr, h->sx_fn.as<StreamFn>(), h->sx_carry.as<StreamCarry>(),
				h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>());
			launch_streams_accept(s, h->rate, (int)S, sb2, h->dev, h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>());
			launch_streams_records(s, h->rate, (int)S, h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>(), h->sxs_first.as<long long>(),
				h->sx_rec.as<SyncState>(), h->sxs_rec_src.as<int>(), (long long)per, (long long)max_rec);
			HIP_OK(hipGetLastError());
		}
		// the call's one host synchronisation: every recording's edge and preamble count plans the records into chunks
		HIP_OK(hipMemcpyAsync(counts.data(), h->sx_counts.p, 2 * S * sizeof(long long), hipMemcpyDeviceToHost, s));
		HIP_OK(hipStreamSynchronize(s));
		long long most = 0;
		for (size_t q = 0; q < S; ++q)
			most = std::max(most, counts[2 * q]);
		if (most <= cap)
			break;
		h->sxs_edge_cap = (long)most;                             // a recording with more falling edges than its share: once more with room for all
	}
	const size_t e2 = mark(h, s);
	h->spans.push_back({ OFDMRX_T_FRONT, e0, e1 });
	h->spans.push_back({ OFDMRX_T_SYNC, e1, e2 });
	size_t at = 0;
	for (size_t q = 0; q < S; ++q) {
		n_pre[q] = (size_t)counts[2 * q + 1];
		first[q] = at;
		at += std::min(n_pre[q], max_per_stream);
	}
	first[S] = at;
	const size_t n_rec = std::min(at, max_records);
	*n_written = n_rec;
	if (n_rec == 0) {
		HIP_OK(hipStreamSynchronize(s));
		return finish_call(h, 0);
	}
	const RecordSources srcs{ h->sxs_rec_src.as<int>(), h->sxs_len.as<int>(), fb2.frame_stride_bytes };
	const FrameBatch all{ fb2.samples, 0, max_len, fb2.fmt, fb2.channels };
	return decode_records(h, all, h->sx_rec.as<SyncState>(), n_rec, out, srcs);
}

// a call that has passed its checks begins: its device, its events and spans, the lengths on the device
int begin_streams(ofdmrx_handle *h, const size_t *n_samples, StreamsCall *call)
{
	HIP_OK(hipSetDevice(h->cfg.device));
	begin_call(h);
	return upload_lengths(h, n_samples, nullptr, call);
}

// the device entries behind their checks: the scan and the records
int streams_device(ofdmrx_handle *h, const void *d_samples, int fmt, int channels, size_t stride, const size_t *n_samples, StreamsCall call,
	size_t max_per_stream, size_t max_records, uint8_t *d_payload_out, ofdmrx_frame_result *d_results, size_t *n_preambles, size_t *first_record)
{
	if (int r = begin_streams(h, n_samples, &call))
		return r;
	size_t n_written = 0;
	return decode_streams_dev(h, FrameBatch{ d_samples, stride, call.max_len, fmt, channels }, call, max_per_stream, max_records,
		Outputs{ d_payload_out, (Result *)d_results, h->esn0_user }, n_preambles, first_record, &n_written);
}

// the host entries behind their checks: the recordings go up, the outputs come back from device staging
int streams_host(ofdmrx_handle *h, const void *samples, int fmt, int channels, size_t stride, const size_t *n_samples, StreamsCall call,
	size_t max_per_stream, size_t max_records, uint8_t *payload_out, ofdmrx_frame_result *results, size_t *n_preambles, size_t *first_record)
{
	const size_t n_streams = call.n_streams;
	int r = begin_streams(h, n_samples, &call);
	if (r)
		return r;
	hipStream_t s = h->stream;
	const size_t frame_bytes = sample_bytes(fmt) * (size_t)channels;
	// the recordings go to the device at the caller's stride, each for its own length: the bytes behind a recording are never read
	r = h->sx_in.ensure(std::max<size_t>(1, n_streams * stride));
	if (r)
		return r;
	for (size_t q = 0; q < n_streams; ++q)
		if (n_samples[q])
			HIP_OK(hipMemcpyAsync((char *)h->sx_in.p + q * stride, (const char *)samples + q * stride, n_samples[q] * frame_bytes, hipMemcpyHostToDevice, s));
	const FrameBatch fb{ h->sx_in.p, stride, call.max_len, fmt, channels };
	// outputs: device staging for as many records as the recordings are likely to hold, copied out behind the call; the Es/N0 rows
	// likewise, in place of the caller's host array
	float *const rows_user = h->esn0_user;
	auto stage = [&](size_t frames) -> int {
		int rr = h->sx_pay.ensure(std::max<size_t>(1, frames) * PAYLOAD_BYTES);
		rr = rr ? rr : h->sx_res.ensure(std::max<size_t>(1, frames) * sizeof(Result));
		const size_t cap = h->sx_pay.bytes / PAYLOAD_BYTES;
		return (rr || !rows_user) ? rr : h->sx_esn0.ensure(std::max<size_t>(1, cap) * ROWS_MAX * sizeof(float));
	};
	auto staged = [&] { return Outputs{ h->sx_pay.as<uint8_t>(), h->sx_res.as<Result>(), rows_user ? h->sx_esn0.as<float>() : nullptr }; };
	// the first guess: 4 records and one per 16384 samples of every recording - more than three for every frame the recording can
	// hold (the shortest frame of the mode table is 64800 samples at 8 kHz)
	size_t guess = 0;
	for (size_t q = 0; q < n_streams; ++q)
		guess += std::min<size_t>(max_per_stream, 4 + n_samples[q] / 16384);
	r = stage(std::min(max_records, guess));
	if (r)
		return r;
	size_t n_rec = 0;
	// a first pass finds how many records there are
	r = decode_streams_dev(h, fb, call, max_per_stream, std::min(max_records, h->sx_pay.bytes / PAYLOAD_BYTES), staged(), n_preambles, first_record, &n_rec);
	if (r)
		return r;
	const size_t want = std::min(first_record[n_streams], max_records);
	if (want > n_rec) {                                           // more records than the staging held: again, with room
		begin_call(h);
		r = stage(want);
		r = r ? r : decode_streams_dev(h, fb, call, max_per_stream, want, staged(), n_preambles, first_record, &n_rec);
		if (r)
			return r;
	}
	if (n_rec) {
		HIP_OK(hipMemcpyAsync(payload_out, h->sx_pay.p, n_rec * PAYLOAD_BYTES, hipMemcpyDeviceToHost, s));
		HIP_OK(hipMemcpyAsync(results, h->sx_res.p, n_rec * sizeof(Result), hipMemcpyDeviceToHost, s));
		if (rows_user)
			HIP_OK(hipMemcpyAsync(rows_user, h->sx_esn0.p, n_rec * ROWS_MAX * sizeof(float), hipMemcpyDeviceToHost, s));
	}
	HIP_OK(hipStreamSynchronize(s));
	return 0;
}

}  // namespace

extern "C" int ofdmrx_decode_streams_device(ofdmrx_handle *h, const void *d_samples, int fmt, int channels, size_t n_streams,
	size_t stride, const size_t *n_samples, size_t max_per_stream, size_t max_records, uint8_t *d_payload_out,
	ofdmrx_frame_result *d_results, size_t *n_preambles, size_t *first_record)
{
	StreamsCall call;
	int r = streams_args(h, d_samples, fmt, channels, n_streams, stride, n_samples, max_records, d_payload_out, d_results, n_preambles, first_record, &call);
	if (r || h->busy_live())                                      // (a handle with an open feed or bank decodes nothing else)
		return OFDMRX_E_ARG;
	return streams_device(h, d_samples, fmt, channels, stride, n_samples, call, max_per_stream, max_records, d_payload_out, d_results, n_preambles, first_record);
}

extern "C" int ofdmrx_decode_streams(ofdmrx_handle *h, const void *samples, int fmt, int channels, size_t n_streams,
	size_t stride, const size_t *n_samples, size_t max_per_stream, size_t max_records, uint8_t *payload_out,
	ofdmrx_frame_result *results, size_t *n_preambles, size_t *first_record)
{
	StreamsCall call;
	int r = streams_args(h, samples, fmt, channels, n_streams, stride, n_samples, max_records, payload_out, results, n_preambles, first_record, &call);
	if (r || h->busy_live())
		return OFDMRX_E_ARG;
	return streams_host(h, samples, fmt, channels, stride, n_samples, call, max_per_stream, max_records, payload_out, results, n_preambles, first_record);
}

extern "C" int ofdmrx_debug_streams_edges(ofdmrx_handle *h, const float *timing, size_t n_streams, const size_t *n, size_t max_edges,
	int64_t *t_edge, int64_t *t_max, int32_t *index_max, size_t *n_edges)
{
	if (!h || !timing || !n || !n_edges || n_streams < 1 || n_streams > 65535)
		return OFDMRX_E_ARG;
	if (max_edges && (!t_edge || !t_max || !index_max))
		return OFDMRX_E_ARG;
	StreamsCall call;
	call.n_streams = n_streams;
	size_t total = 0;
	for (size_t q = 0; q < n_streams; ++q) {
		if (n[q] > (size_t)0x7fffffff / 2)
			return OFDMRX_E_ARG;
		call.max_len = std::max(call.max_len, (long)n[q]);
		total += n[q];
	}
	HIP_OK(hipSetDevice(h->cfg.device));
	hipStream_t s = h->stream;
	std::fill(n_edges, n_edges + n_streams, (size_t)0);
	if (call.max_len == 0)
		return 0;
	int r = upload_lengths(h, n, n, &call);
	const long cap = (long)std::max<size_t>(1, max_edges);
	r = r ? r : h->sx_timing.ensure(total * sizeof(float));
	r = r ? r : h->sx_fn.ensure((size_t)call.total_tiles * sizeof(StreamFn));
	r = r ? r : h->sx_carry.ensure((size_t)call.total_tiles * sizeof(StreamCarry));
	r = r ? r : h->sx_edges.ensure(n_streams * (size_t)cap * sizeof(StreamEdge));
	if (r)
		return r;
	HIP_OK(hipMemcpyAsync(h->sx_timing.p, timing, total * sizeof(float), hipMemcpyHostToDevice, s));
	HIP_OK(hipMemsetAsync(h->sx_counts.p, 0, 2 * n_streams * sizeof(long long), s));
	launch_streams_scan(s, h->rate, (int)n_streams, call.max_len, source_batch(h, FrameBatch{ nullptr, 0, call.max_len, OFDMRX_FMT_F32, 2 }),
		h->sx_timing.as<float>(), h->sx_fn.as<StreamFn>(), h->sx_carry.as<StreamCarry>(), h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>());
	HIP_OK(hipGetLastError());
	std::vector<long long> &counts = h->sxs_counts_h;
	counts.assign(2 * n_streams, 0);
	HIP_OK(hipMemcpyAsync(counts.data(), h->sx_counts.p, 2 * n_streams * sizeof(long long), hipMemcpyDeviceToHost, s));
	HIP_OK(hipStreamSynchronize(s));
	std::vector<StreamEdge> e(max_edges ? n_streams * (size_t)cap : 0);
	if (!e.empty())
		HIP_OK(hipMemcpy(e.data(), h->sx_edges.p, e.size() * sizeof(StreamEdge), hipMemcpyDeviceToHost));
	for (size_t q = 0; q < n_streams; ++q) {
		n_edges[q] = (size_t)counts[2 * q];
		const size_t w = std::min<size_t>(n_edges[q], max_edges);
		for (size_t i = 0; i < w; ++i) {
			const StreamEdge &ed = e[q * (size_t)cap + i];
			t_edge[q * max_edges + i] = ed.g;
			t_max[q * max_edges + i] = ed.t_max;
			index_max[q * max_edges + i] = ed.index_max;
		}
	}
	return 0;
}

// ---- one recording: a batch of one.  The recording is the batch's only one, a whole number of sample frames apart from a next
// that does not exist; every record may be its own (max_per_stream = max_records = max_frames).  What these entries refuse and the
// batched ones take - an empty recording, an empty sequence - is refused here, before the handle is looked at.
namespace {

int one_stream_args(ofdmrx_handle *h, const void *samples, int fmt, int channels, size_t n_samples, size_t max_frames, const void *payload,
	const void *results, size_t *n_preambles, size_t *first, size_t *stride, StreamsCall *call)
{
	if (n_samples == 0 || n_samples > (size_t)0x7fffffff / 2)
		return OFDMRX_E_ARG;
	*stride = n_samples * sample_bytes(fmt) * (size_t)channels;
	int r = streams_args(h, samples, fmt, channels, 1, *stride, &n_samples, max_frames, payload, results, n_preambles, first, call);
	return (r || h->busy_live()) ? OFDMRX_E_ARG : 0;
}

}  // namespace

extern "C" int ofdmrx_decode_stream_device(ofdmrx_handle *h, const void *d_samples, int fmt, int channels, size_t n_samples,
	size_t max_frames, uint8_t *d_payload_out, ofdmrx_frame_result *d_results, size_t *n_preambles)
{
	StreamsCall call;
	size_t stride = 0, first[2];
	if (int r = one_stream_args(h, d_samples, fmt, channels, n_samples, max_frames, d_payload_out, d_results, n_preambles, first, &stride, &call))
		return r;
	return streams_device(h, d_samples, fmt, channels, stride, &n_samples, call, max_frames, max_frames, d_payload_out, d_results, n_preambles, first);
}

extern "C" int ofdmrx_decode_stream(ofdmrx_handle *h, const void *samples, int fmt, int channels, size_t n_samples,
	size_t max_frames, uint8_t *payload_out, ofdmrx_frame_result *results, size_t *n_preambles)
{
	StreamsCall call;
	size_t stride = 0, first[2], n_pre = 0;
	if (int r = one_stream_args(h, samples, fmt, channels, n_samples, max_frames, payload_out, results, n_preambles, first, &stride, &call))
		return r;
	if (int r = streams_host(h, samples, fmt, channels, stride, &n_samples, call, max_frames, max_frames, payload_out, results, &n_pre, first))
		return r;
	*n_preambles = n_pre;                                         // (written when the call has succeeded, outputs copied)
	return 0;
}

extern "C" int ofdmrx_debug_stream_edges(ofdmrx_handle *h, const float *timing, size_t n, size_t max_edges,
	int64_t *t_edge, int64_t *t_max, int32_t *index_max, size_t *n_edges)
{
	if (n == 0)
		return OFDMRX_E_ARG;
	return ofdmrx_debug_streams_edges(h, timing, 1, &n, max_edges, t_edge, t_max, index_max, n_edges);
}
