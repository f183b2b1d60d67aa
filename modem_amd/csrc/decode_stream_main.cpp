// decode_stream_main.cpp -- `decode_stream [--live] OUTDIR INPUT`: every frame of a recording.
// OUTDIR/<k>.dat holds the 5380 bytes `decode OUT INPUT k` writes (descrambled; zeros for a failed frame), for every preamble k
// the SKIP loop of decode.cc:390-448 would count; one summary line per record on stderr.  Exit status 0 like `decode`
// (decode.cc:619), 1 on argument, WAV or library errors.
// Without --live the whole recording is read and decoded in one call (ofdmrx_decode_stream).  With --live the WAV header is read,
// then the body in blocks of one second as it arrives (INPUT `-`: standard input, e.g. a recorder's pipe), every block is pushed into
// a feed (ofdmrx_feed_*) and every record is written as soon as it is returned: the same files and lines, each when its frame is in.
// `decode_stream --batch OUTROOT A.wav B.wav ...`: many recordings in one call (ofdmrx_decode_streams).  Recording i goes to
// OUTROOT/<i>/<k>.dat (the directories are made) and its summary lines are the one-call lines prefixed with `<i>:`.  The inputs must
// share sample rate, channel count and sample format.
// `decode_stream --live --batch OUTROOT A.wav B.wav ...`: the same recordings read in blocks of one second, in lock step, and pushed
// through one bank of live channels (ofdmrx_bank_*); a file that runs out ends its channel.  Every record is written as soon as it
// is returned: the files and lines of --batch, up to the order of the lines.
// `decode_stream --wideband DECIM F1,F2,... OUTROOT WIDE.wav`: one wideband I/Q capture (2 channels, DECIM x a supported rate) read
// in blocks of one wideband second and pushed through a wideband bank (ofdmrx_bank_begin_wideband): channel i, centred at Fi Hz, goes
// to OUTROOT/<i>/<k>.dat with the `<i>:` summary lines of --live --batch.
// `decode_stream --wideband DECIM auto OUTROOT WIDE.wav`: the capture is surveyed first (ofdmrx_util_survey over the whole file, 1280
// bins, and ofdmrx_util_find_bands with its default parameters: what `survey WIDE.wav DECIM` prints), the centres found are printed
// on stderr, and then exactly the form above runs with that list.  The file is read twice, so `auto` does not take standard input.
// DECIM may be a ratio P/Q in both forms - it is one when it holds a '/' (Q <= 16, 2 <= P / Q <= 32): the
// capture's rate x Q / P must be a supported rate, and the bank is opened with ofdmrx_bank_begin_wideband_ratio.
// `decode_stream --wideband-real DECIM|P/Q F1,F2,... OUTROOT MONO.wav`: the same for a REAL capture (DESIGN.md section 4.25,
// ofdmrx_bank_begin_wideband_real) - a ONE-channel file, a sound-card recording of a receiver's audio or IF - read in blocks of one
// wideband second.  A centre with |F| < rate / 4 or |F| > capture rate / 2 - rate / 4 is refused by the library.  A two-channel file
// is refused (that is `--wideband`), and so is `auto`: the survey of a real capture is not built.  The `--wideband` forms keep turning
// a one-channel file away.
// `decode_stream --grid DECIM K1,K2,...|all OUTROOT WIDE.wav`: the same through the grid front end (DESIGN.md section 4.19,
// ofdmrx_bank_begin_wideband_grid): DECIM a power of two 2 .. 512, the capture's rate DECIM x a supported rate, channel i the slot Ki
// (-DECIM .. DECIM - 1; `all`: every slot in ascending order) centred at Ki x rate / 2.  Every opened slot's centre is printed on
// stderr first; the files and lines are those of --wideband.
// `decode_stream --grid P/Q K1,K2,...|all OUTROOT WIDE.wav`: the grid front end at a ratio (DESIGN.md section 4.22,
// ofdmrx_bank_begin_wideband_grid_ratio): the spelling with '/' - 6/1 is a 48 kHz capture at an 8 kHz handle; the slots are the K with
// -P <= K Q < P.  A bare integer keeps the power-of-two rule.  `--grid P/Q auto` is refused: under --grid the grid survey at a ratio is
// not built; it is `--grid-ratio P/Q auto`, below.
// `decode_stream --grid DECIM auto[:FLOOR_DB] OUTROOT WIDE.wav`: the capture is surveyed first (what `survey
// --grid WIDE.wav DECIM [FLOOR_DB]` prints), the slots found are printed on stderr, and then exactly the form above runs with that
// list.  The file is read twice, so `auto` does not take standard input; no slot found is an error.
// `decode_stream --grid-ratio P/Q K1,K2,...|all|auto[:FLOOR_DB] OUTROOT WIDE.wav`: a list or `all` is `--grid P/Q` exactly; `auto`
// surveys the capture first (what `survey --grid-ratio WIDE.wav P/Q [FLOOR_DB]` prints) and then runs that form.
#include "survey_cli.h"
#include <algorithm>
#include <cstdlib>
#include <string>
#include <sys/stat.h>

// one record: its line on stderr, its file
static bool emit_record(const std::string &outdir, size_t k, const ofdmrx_frame_result &q, const uint8_t *payload, const char *prefix = "")
{
	static const char *names[] = { "ok", "no sync", "OSD error", "header CRC error", "mode unsupported", "call sign unsupported",
		"payload decoding error" };
	char cs[10];
	unsigned long long v = q.call_sign;
	for (int i = 8; i >= 0; --i, v /= 37)                         // base37_decoder, decode.cc:155-159
		cs[i] = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"[v % 37];
	cs[9] = 0;
	std::fprintf(stderr, "%s%zu: sample %lld mode %d call sign %s %s bit flips %d\n", prefix, k, (long long)q.sc_start, q.oper_mode, cs,
		q.status >= 0 && q.status <= 6 ? names[q.status] : "?", q.bit_flips);
	const std::string name = outdir + "/" + std::to_string(k) + ".dat";
	FILE *f = std::fopen(name.c_str(), "wb");
	if (!f) {
		std::fprintf(stderr, "Couldn't open file \"%s\" for writing.\n", name.c_str());
		return false;
	}
	std::fwrite(payload, 1, OFDMRX_PAYLOAD_BYTES, f);
	std::fclose(f);
	return true;
}

static bool supported(int channels, int rate)
{
	if (channels < 1 || channels > 2) {
		std::fprintf(stderr, "Only real or analytic signal (one or two channels) supported.\n");
		return false;
	}
	if (rate != 8000 && rate != 16000 && rate != 44100 && rate != 48000) {   // decode.cc:590-605
		std::fprintf(stderr, "Unsupported sample rate.\n");
		return false;
	}
	if (ofdmrx_abi_version() != OFDMRX_ABI_VERSION || ofdmrx_abi_minor() < 7) {
		std::fprintf(stderr, "libofdmrx: ABI %d.%d, this program needs %d.7\n", ofdmrx_abi_version(), ofdmrx_abi_minor(), OFDMRX_ABI_VERSION);
		return false;
	}
	return true;
}

static ofdmrx_handle *create(int rate)
{
	ofdmrx_config cfg{};
	cfg.abi_version = OFDMRX_ABI_VERSION;
	cfg.sample_rate = rate;
	cfg.list_size = 8;
	cfg.device = 0;
	cfg.chunk_frames = 64;
	cfg.descramble = 1;
	ofdmrx_handle *h = nullptr;
	const int r = ofdmrx_create(&cfg, &h);
	if (r) {
		std::fprintf(stderr, "ofdmrx_create: %s\n", ofdmrx_strerror(r));
		return nullptr;
	}
	return h;
}

// the body block by block through a feed
static int run_live(const std::string &outdir, const char *input_name)
{
	WavStream w;
	if (!wav_open(input_name, w)) {
		std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", input_name);
		return 1;
	}
	if (!supported(w.channels, w.rate))
		return 1;
	ofdmrx_handle *h = create(w.rate);
	if (!h)
		return 1;
	int r = ofdmrx_feed_begin(h, w.fmt, w.channels);
	const size_t cap = 64;
	std::vector<uint8_t> out(cap * OFDMRX_PAYLOAD_BYTES), pcm;
	std::vector<ofdmrx_frame_result> res(cap);
	size_t k = 0, total = 0;
	bool written = true;
	// one push (or the end of the feed) and every record it makes ready: when more are ready than the arrays hold, further calls
	// without samples take the rest
	auto step = [&](bool end, const void *samples, size_t n) -> int {
		size_t n_rec = 0, n_left = 0;
		do {
			const int rr = end ? ofdmrx_feed_end(h, cap, out.data(), res.data(), &n_rec, &n_left)
				: ofdmrx_feed_push(h, samples, n, cap, out.data(), res.data(), &n_rec, &n_left);
			if (rr)
				return rr;
			samples = nullptr;
			n = 0;
			for (size_t i = 0; i < n_rec && written; ++i, ++k)
				written = emit_record(outdir, k, res[i], out.data() + i * OFDMRX_PAYLOAD_BYTES);
		} while (n_left && written);
		return 0;
	};
	for (bool last = false; !r && written && !last;) {
		const size_t n = wav_read_block(w, (size_t)w.rate, pcm);  // one second; fewer at the end of the body
		total += n;
		last = n < (size_t)w.rate;
		if (n)
			r = step(false, pcm.data(), n);
	}
	if (!r && written && total == 0) {
		std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", input_name);
		written = false;
	}
	if (!r && written)
		r = step(true, nullptr, 0);
	if (r)
		std::fprintf(stderr, "ofdmrx_feed: %s\n", ofdmrx_strerror(r));
	ofdmrx_destroy(h);
	return (r || !written) ? 1 : 0;
}

// every recording of a list in one call
static int run_batch(const std::string &outroot, int n_inputs, char **inputs)
{
	std::vector<Wav> wavs((size_t)n_inputs);
	size_t longest = 0;
	for (int i = 0; i < n_inputs; ++i) {
		if (!read_wav(inputs[i], wavs[i])) {                      // (a WAV without sample frames is a recording of length 0: no records)
			std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", inputs[i]);
			return 1;
		}
		if (wavs[i].rate != wavs[0].rate || wavs[i].channels != wavs[0].channels || wavs[i].fmt != wavs[0].fmt) {
			std::fprintf(stderr, "\"%s\" and \"%s\" do not share sample rate, channels and sample format: a batch takes recordings of one kind.\n",
				inputs[0], inputs[i]);
			return 1;
		}
		longest = std::max(longest, wavs[i].frames);
	}
	const Wav &w0 = wavs[0];
	if (!supported(w0.channels, w0.rate))
		return 1;
	const size_t S = (size_t)n_inputs, frame_bytes = (w0.fmt == OFDMRX_FMT_S16 ? 2 : w0.fmt == OFDMRX_FMT_U8 ? 1 : 4) * (size_t)w0.channels;
	const size_t stride = std::max<size_t>(longest, 1) * frame_bytes;
	std::vector<uint8_t> all(S * stride);
	std::vector<size_t> lens(S), n_pre(S), first(S + 1);
	for (size_t i = 0; i < S; ++i) {
		lens[i] = wavs[i].frames;
		std::memcpy(all.data() + i * stride, wavs[i].pcm.data(), lens[i] * frame_bytes);
		wavs[i].pcm = std::vector<uint8_t>();
	}
	ofdmrx_handle *h = create(w0.rate);
	if (!h)
		return 1;
	size_t cap = 64 * S;
	std::vector<uint8_t> out;
	std::vector<ofdmrx_frame_result> res;
	for (;;) {                                                    // a second call only when the recordings hold more than the first guess
		out.assign(cap * OFDMRX_PAYLOAD_BYTES, 0);
		res.assign(cap, ofdmrx_frame_result{});
		const int r = ofdmrx_decode_streams(h, all.data(), w0.fmt, w0.channels, S, stride, lens.data(), (size_t)-1, cap, out.data(), res.data(),
			n_pre.data(), first.data());
		if (r) {
			std::fprintf(stderr, "ofdmrx_decode_streams: %s\n", ofdmrx_strerror(r));
			ofdmrx_destroy(h);
			return 1;
		}
		if (first[S] <= cap)
			break;
		cap = first[S];
	}
	ofdmrx_destroy(h);
	(void)mkdir(outroot.c_str(), 0777);
	for (size_t i = 0; i < S; ++i) {
		const std::string dir = outroot + "/" + std::to_string(i), prefix = std::to_string(i) + ":";
		(void)mkdir(dir.c_str(), 0777);
		for (size_t k = first[i]; k < first[i + 1]; ++k)
			if (!emit_record(dir, k - first[i], res[k], out.data() + k * OFDMRX_PAYLOAD_BYTES, prefix.c_str()))
				return 1;
	}
	return 0;
}

// every recording of a list block by block, in lock step, through one bank
static int run_live_batch(const std::string &outroot, int n_inputs, char **inputs)
{
	const size_t S = (size_t)n_inputs;
	std::vector<WavStream> ws(S);
	for (size_t i = 0; i < S; ++i) {
		if (!wav_open(inputs[i], ws[i])) {
			std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", inputs[i]);
			return 1;
		}
		if (ws[i].rate != ws[0].rate || ws[i].channels != ws[0].channels || ws[i].fmt != ws[0].fmt) {
			std::fprintf(stderr, "\"%s\" and \"%s\" do not share sample rate, channels and sample format: a batch takes recordings of one kind.\n",
				inputs[0], inputs[i]);
			return 1;
		}
	}
	const WavStream &w0 = ws[0];
	if (!supported(w0.channels, w0.rate))
		return 1;
	if (S > 65535) {
		std::fprintf(stderr, "A bank takes at most 65535 recordings.\n");
		return 1;
	}
	ofdmrx_handle *h = create(w0.rate);
	if (!h)
		return 1;
	(void)mkdir(outroot.c_str(), 0777);
	std::vector<std::string> dirs(S), prefixes(S);
	for (size_t i = 0; i < S; ++i) {
		dirs[i] = outroot + "/" + std::to_string(i);
		prefixes[i] = std::to_string(i) + ":";
		(void)mkdir(dirs[i].c_str(), 0777);
	}
	int r = ofdmrx_bank_begin(h, S, w0.fmt, w0.channels);
	const size_t block = (size_t)w0.rate, frame_bytes = (w0.fmt == OFDMRX_FMT_S16 ? 2 : w0.fmt == OFDMRX_FMT_U8 ? 1 : 4) * (size_t)w0.channels;
	const size_t stride = block * frame_bytes, cap = 64;
	std::vector<uint8_t> all(S * stride), out(cap * OFDMRX_PAYLOAD_BYTES), pcm, ends(S), over(S, 0);
	std::vector<ofdmrx_frame_result> res(cap);
	std::vector<int32_t> chan(cap);
	std::vector<int64_t> index(cap);
	std::vector<size_t> lens(S), none(S, 0);
	bool written = true;
	auto step = [&](bool end) -> int {
		size_t n_rec = 0, n_left = 0;
		bool first = true;
		do {
			const int rr = end ? ofdmrx_bank_end(h, cap, out.data(), res.data(), chan.data(), index.data(), &n_rec, &n_left)
				: ofdmrx_bank_push(h, first ? all.data() : nullptr, stride, first ? lens.data() : none.data(), first ? ends.data() : nullptr, cap,
					out.data(), res.data(), chan.data(), index.data(), &n_rec, &n_left);
			if (rr)
				return rr;
			first = false;
			for (size_t i = 0; i < n_rec && written; ++i)
				written = emit_record(dirs[(size_t)chan[i]], (size_t)index[i], res[i], out.data() + i * OFDMRX_PAYLOAD_BYTES, prefixes[(size_t)chan[i]].c_str());
		} while (n_left && written);
		return 0;
	};
	for (size_t open = S; !r && written && open;) {
		for (size_t i = 0; i < S; ++i) {
			lens[i] = 0;
			ends[i] = 0;
			if (over[i])
				continue;
			lens[i] = wav_read_block(ws[i], block, pcm);
			std::memcpy(all.data() + i * stride, pcm.data(), lens[i] * frame_bytes);
			if (lens[i] < block) {                                    // the file has run out: its channel ends behind these samples
				ends[i] = over[i] = 1;
				--open;
			}
		}
		r = step(false);
	}
	if (!r && written)
		r = step(true);
	if (r)
		std::fprintf(stderr, "ofdmrx_bank: %s\n", ofdmrx_strerror(r));
	ofdmrx_destroy(h);
	for (WavStream &w : ws)
		if (w.f)
			std::fclose(w.f);
	return (r || !written) ? 1 : 0;
}

// the centres of the occupied bands of a capture, as the list run_wideband takes ("" with a message: none, or an error)
static std::string survey_centres(const Decimation &decim, const char *input_name)
{
	if (!std::strcmp(input_name, "-") || !std::strcmp(input_name, "/dev/stdin")) {
		std::fprintf(stderr, "`auto` reads the capture twice: give a file, not standard input.\n");
		return "";
	}
	Wav w;
	if (!read_wav(input_name, w) || w.frames == 0) {
		std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", input_name);
		return "";
	}
	if (w.channels != 2) {
		std::fprintf(stderr, "A wideband capture is an analytic signal (two channels).\n");
		return "";
	}
	if (!decim.valid() || !decim.rate_of(w.rate) || !supported(2, decim.rate_of(w.rate))) {
		if (!decim.valid() || !decim.rate_of(w.rate))
			std::fprintf(stderr, "Unsupported sample rate.\n");
		return "";
	}
	ofdmrx_handle *h = create(decim.rate_of(w.rate));
	if (!h)
		return "";
	std::vector<ofdmrx_band> bands;
	double floor = 0.0;
	const bool ok = survey_capture(h, w, 1280, bands, floor);
	ofdmrx_destroy(h);
	if (!ok)
		return "";
	if (bands.empty()) {
		std::fprintf(stderr, "The survey found no occupied band (floor %.6g).\n", floor);
		return "";
	}
	std::string list;
	for (const ofdmrx_band &b : bands) {
		char t[40];
		std::snprintf(t, sizeof(t), "%s%.17g", list.empty() ? "" : ",", b.centre_hz);
		list += t;
	}
	std::fprintf(stderr, "survey: floor %.6g, centres %s\n", floor, list.c_str());
	return list;
}

// the occupied slots of a grid capture, as the list run_wideband takes with grid = true ("" with a message: none, or an error).
// how: `auto` or `auto:FLOOR_DB`; at_ratio: `--grid-ratio P/Q auto`
static std::string survey_slots(const char *decim_arg, const char *how, const char *input_name, bool at_ratio = false)
{
	if (!std::strcmp(input_name, "-") || !std::strcmp(input_name, "/dev/stdin")) {
		std::fprintf(stderr, "`auto` reads the capture twice: give a file, not standard input.\n");
		return "";
	}
	const int decim = std::atoi(decim_arg);
	double abs_floor = 0.0;
	const Decimation ratio(decim_arg);
	if (!at_ratio && std::strchr(decim_arg, '/')) {
		std::fprintf(stderr, "The grid survey at a ratio P/Q is not built under --grid: `--grid P/Q auto` is refused; use `--grid-ratio P/Q auto[:FLOOR_DB]`, name the slots or give `all`.\n");
		return "";
	}
	int32_t k_first = 0;
	size_t n_all = 0;
	if (at_ratio && (!ratio.ratio || ratio.p <= 0 || ratio.q <= 0 || ofdmrx_util_grid_ratio_slots(ratio.p, ratio.q, &k_first, &n_all))) {
		std::fprintf(stderr, "A grid bank at a ratio takes P/Q with, in lowest terms, Q 1 .. 16 and P 2 Q .. 512 with no prime factor other than 2, 3 and 5.\n");
		return "";
	}
	if (!at_ratio && !grid_decim_valid(decim)) {
		std::fprintf(stderr, "A grid bank takes a decimation that is a power of two 2 .. 512.\n");
		return "";
	}
	if (how[4] && !survey_floor_arg(how + 5, abs_floor)) {
		std::fprintf(stderr, "`auto:FLOOR_DB` takes a floor in dB re full scale.\n");
		return "";
	}
	Wav w;
	if (!read_wav(input_name, w) || w.frames == 0) {
		std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", input_name);
		return "";
	}
	if (w.channels != 2) {
		std::fprintf(stderr, "A wideband capture is an analytic signal (two channels).\n");
		return "";
	}
	const int rate = at_ratio ? ratio.rate_of(w.rate) : w.rate % decim ? 0 : w.rate / decim;
	if (!rate || !supported(2, rate)) {
		if (!rate)
			std::fprintf(stderr, "Unsupported sample rate.\n");
		return "";
	}
	ofdmrx_handle *h = create(rate);
	if (!h)
		return "";
	std::vector<ofdmrx_slot> slots;
	double floor = 0.0;
	const bool ok = at_ratio ? survey_grid_ratio_capture(h, w, ratio.p, ratio.q, abs_floor, slots, floor) : survey_grid_capture(h, w, decim, abs_floor, slots, floor);
	ofdmrx_destroy(h);
	if (!ok)
		return "";
	if (slots.empty()) {
		std::fprintf(stderr, "The survey found no occupied slot (floor %.6g).\n", floor);
		return "";
	}
	std::string list;
	for (const ofdmrx_slot &s : slots)
		list += (list.empty() ? "" : ",") + std::to_string(s.slot);
	std::fprintf(stderr, "survey: floor %.6g, slots %s\n", floor, list.c_str());
	return list;
}

// one wideband capture block by block through a wideband bank (grid: through a grid bank - centre_list holds slot numbers, or `all`;
// real: a one-channel capture through the bank for a real capture, not with grid)
static int run_wideband(const Decimation &decim, const char *centre_list, const std::string &outroot, const char *input_name, bool grid = false,
	bool real = false)
{
	std::vector<double> centres;
	std::vector<int32_t> slots;
	if (grid) {
		// a bare integer keeps the power-of-two rule; the spelling P/Q is the grid front end at a ratio
		int32_t k_first = -decim.p;
		size_t n_all = 2 * (size_t)(decim.p > 0 ? decim.p : 0);
		if (decim.ratio && ofdmrx_util_grid_ratio_slots(decim.p, decim.q, &k_first, &n_all)) {
			std::fprintf(stderr, "A grid bank at a ratio takes P/Q with, in lowest terms, Q 1 .. 16 and P 2 Q .. 512 with no prime factor other than 2, 3 and 5.\n");
			return 1;
		}
		if (!decim.ratio && (decim.p < 2 || decim.p > 512 || (decim.p & (decim.p - 1)))) {
			std::fprintf(stderr, "A grid bank takes a decimation that is a power of two 2 .. 512.\n");
			return 1;
		}
		const long k_last = (long)k_first + (long)n_all - 1;
		if (!std::strcmp(centre_list, "all")) {
			for (long k = k_first; k <= k_last; ++k)
				slots.push_back((int32_t)k);
		} else {
			for (const char *p = centre_list; *p;) {
				char *e = nullptr;
				const long k = std::strtol(p, &e, 10);
				if (e == p || (*e && *e != ',') || k < k_first || k > k_last) {
					std::fprintf(stderr, "Slots are `all` or a comma-separated list of numbers %d .. %ld.\n", (int)k_first, k_last);
					return 1;
				}
				slots.push_back((int32_t)k);
				p = *e ? e + 1 : e;
			}
		}
		if (slots.empty() || slots.size() > 65535) {
			std::fprintf(stderr, "A grid bank takes 1 .. 65535 slots.\n");
			return 1;
		}
		centres.assign(slots.size(), 0.0);                            // (filled in below, once the rate is known)
		centre_list = "";
	}
	for (const char *p = centre_list; *p;) {
		char *e = nullptr;
		const double f = std::strtod(p, &e);
		if (e == p || (*e && *e != ',')) {
			std::fprintf(stderr, "Centre frequencies are a comma-separated list of Hz.\n");
			return 1;
		}
		centres.push_back(f);
		p = *e ? e + 1 : e;
	}
	if ((!grid && !decim.valid()) || centres.empty() || centres.size() > 65535) {
		std::fprintf(stderr, "A wideband bank takes a decimation of 2 .. 32 (a ratio P/Q: Q <= 16) and 1 .. 65535 centre frequencies.\n");
		return 1;
	}
	WavStream w;
	if (!wav_open(input_name, w)) {
		std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", input_name);
		return 1;
	}
	if (real && w.channels != 1) {
		std::fprintf(stderr, "--wideband-real takes a real capture (one channel); an analytic capture (two channels) is `--wideband`.\n");
		return 1;
	}
	if (!real && w.channels != 2) {
		std::fprintf(stderr, "A wideband capture is an analytic signal (two channels).\n");
		return 1;
	}
	if (!decim.rate_of(w.rate) || !supported(2, decim.rate_of(w.rate))) {
		if (!decim.rate_of(w.rate))
			std::fprintf(stderr, "Unsupported sample rate.\n");
		return 1;
	}
	ofdmrx_handle *h = create(decim.rate_of(w.rate));
	if (!h)
		return 1;
	const size_t S = centres.size(), cap = 64;
	(void)mkdir(outroot.c_str(), 0777);
	std::vector<std::string> dirs(S), prefixes(S);
	for (size_t i = 0; i < S; ++i) {
		dirs[i] = outroot + "/" + std::to_string(i);
		prefixes[i] = std::to_string(i) + ":";
		(void)mkdir(dirs[i].c_str(), 0777);
	}
	for (size_t i = 0; i < S && grid; ++i) {
		centres[i] = (double)slots[i] * 0.5 * (double)decim.rate_of(w.rate);
		std::fprintf(stderr, "%zu: slot %d, centre %.17g Hz\n", i, (int)slots[i], centres[i]);
	}
	int r = real ? ofdmrx_bank_begin_wideband_real(h, S, centres.data(), decim.p, decim.q, w.fmt)
		: grid && decim.ratio ? ofdmrx_bank_begin_wideband_grid_ratio(h, S, slots.data(), decim.p, decim.q, w.fmt)
		: grid ? ofdmrx_bank_begin_wideband_grid(h, S, slots.data(), decim.p, w.fmt)
		: decim.ratio ? ofdmrx_bank_begin_wideband_ratio(h, S, centres.data(), decim.p, decim.q, w.fmt)
		: ofdmrx_bank_begin_wideband(h, S, centres.data(), decim.p, w.fmt);
	std::vector<uint8_t> out(cap * OFDMRX_PAYLOAD_BYTES), pcm;
	std::vector<ofdmrx_frame_result> res(cap);
	std::vector<int32_t> chan(cap);
	std::vector<int64_t> index(cap);
	bool written = true;
	auto step = [&](bool end, const void *samples, size_t n) -> int {
		size_t n_rec = 0, n_left = 0;
		do {
			const int rr = end ? ofdmrx_bank_end(h, cap, out.data(), res.data(), chan.data(), index.data(), &n_rec, &n_left)
				: ofdmrx_bank_push_wideband(h, samples, n, 0, cap, out.data(), res.data(), chan.data(), index.data(), &n_rec, &n_left);
			if (rr)
				return rr;
			samples = nullptr;
			n = 0;
			for (size_t i = 0; i < n_rec && written; ++i)
				written = emit_record(dirs[(size_t)chan[i]], (size_t)index[i], res[i], out.data() + i * OFDMRX_PAYLOAD_BYTES, prefixes[(size_t)chan[i]].c_str());
		} while (n_left && written);
		return 0;
	};
	for (bool last = false; !r && written && !last;) {
		const size_t n = wav_read_block(w, (size_t)w.rate, pcm);      // one wideband second; fewer at the end of the body
		last = n < (size_t)w.rate;
		if (n)
			r = step(false, pcm.data(), n);
	}
	if (!r && written)
		r = step(true, nullptr, 0);
	if (r)
		std::fprintf(stderr, "ofdmrx_bank: %s\n", ofdmrx_strerror(r));
	ofdmrx_destroy(h);
	if (w.f)
		std::fclose(w.f);
	return (r || !written) ? 1 : 0;
}

int main(int argc, char **argv)
{
	if (argc == 6 && !std::strcmp(argv[1], "--wideband") && !std::strcmp(argv[3], "auto")) {
		const std::string found = survey_centres(Decimation(argv[2]), argv[5]);
		return found.empty() ? 1 : run_wideband(Decimation(argv[2]), found.c_str(), argv[4], argv[5]);
	}
	if (argc == 6 && !std::strcmp(argv[1], "--wideband"))
		return run_wideband(Decimation(argv[2]), argv[3], argv[4], argv[5]);
	if (argc == 6 && !std::strcmp(argv[1], "--wideband-real")) {
		if (!std::strncmp(argv[3], "auto", 4) && (!argv[3][4] || argv[3][4] == ':')) {
			std::fprintf(stderr, "The survey of a real capture is not built: `--wideband-real DECIM auto` is refused; name the centre frequencies.\n");
			return 1;
		}
		return run_wideband(Decimation(argv[2]), argv[3], argv[4], argv[5], false, true);
	}
	if (argc == 6 && !std::strcmp(argv[1], "--grid") && !std::strncmp(argv[3], "auto", 4) && (!argv[3][4] || argv[3][4] == ':')) {
		const std::string found = survey_slots(argv[2], argv[3], argv[5]);
		return found.empty() ? 1 : run_wideband(Decimation(argv[2]), found.c_str(), argv[4], argv[5], true);
	}
	if (argc == 6 && !std::strcmp(argv[1], "--grid"))
		return run_wideband(Decimation(argv[2]), argv[3], argv[4], argv[5], true);
	if (argc == 6 && !std::strcmp(argv[1], "--grid-ratio")) {
		if (!Decimation(argv[2]).ratio) {
			std::fprintf(stderr, "--grid-ratio takes a ratio P/Q (the spelling with '/'); a power of two is `--grid DECIM`.\n");
			return 1;
		}
		if (!std::strncmp(argv[3], "auto", 4) && (!argv[3][4] || argv[3][4] == ':')) {
			const std::string found = survey_slots(argv[2], argv[3], argv[5], true);
			return found.empty() ? 1 : run_wideband(Decimation(argv[2]), found.c_str(), argv[4], argv[5], true);
		}
		return run_wideband(Decimation(argv[2]), argv[3], argv[4], argv[5], true);
	}
	if (argc >= 5 && !std::strcmp(argv[1], "--live") && !std::strcmp(argv[2], "--batch"))
		return run_live_batch(argv[3], argc - 4, argv + 4);
	if (argc >= 4 && !std::strcmp(argv[1], "--batch"))
		return run_batch(argv[2], argc - 3, argv + 3);
	const bool live = argc == 4 && !std::strcmp(argv[1], "--live");
	if (argc != 3 && !live) {
		std::fprintf(stderr, "usage: %s [--live] OUTDIR INPUT\n       %s [--live] --batch OUTROOT INPUT...\n       %s --wideband DECIM|P/Q F1,F2,...|auto OUTROOT INPUT\n       %s --wideband-real DECIM|P/Q F1,F2,... OUTROOT MONO_INPUT\n       %s --grid DECIM|P/Q K1,K2,...|all|auto[:FLOOR_DB] OUTROOT INPUT\n       %s --grid-ratio P/Q K1,K2,...|all|auto[:FLOOR_DB] OUTROOT INPUT\n",
			argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
		return 1;
	}
	const std::string outdir = argv[live ? 2 : 1];
	const char *input_name = argv[live ? 3 : 2];
	if (!std::strcmp(input_name, "-"))
		input_name = "/dev/stdin";
	if (live)
		return run_live(outdir, input_name);
	Wav w;
	if (!read_wav(input_name, w) || w.frames == 0) {
		std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", input_name);
		return 1;
	}
	if (!supported(w.channels, w.rate))
		return 1;
	ofdmrx_handle *h = create(w.rate);
	if (!h)
		return 1;
	size_t cap = 64, n_pre = 0;
	std::vector<uint8_t> out;
	std::vector<ofdmrx_frame_result> res;
	for (;;) {                                                    // a second call only when the recording holds more than the first guess
		out.assign(cap * OFDMRX_PAYLOAD_BYTES, 0);
		res.assign(cap, ofdmrx_frame_result{});
		const int r = ofdmrx_decode_stream(h, w.pcm.data(), w.fmt, w.channels, w.frames, cap, out.data(), res.data(), &n_pre);
		if (r) {
			std::fprintf(stderr, "ofdmrx_decode_stream: %s\n", ofdmrx_strerror(r));
			ofdmrx_destroy(h);
			return 1;
		}
		if (n_pre <= cap)
			break;
		cap = n_pre;
	}
	ofdmrx_destroy(h);
	for (size_t k = 0; k < n_pre; ++k)
		if (!emit_record(outdir, k, res[k], out.data() + k * OFDMRX_PAYLOAD_BYTES))
			return 1;
	return 0;
}
