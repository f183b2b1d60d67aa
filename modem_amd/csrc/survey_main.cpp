// survey_main.cpp -- `survey WIDE.wav DECIM|P/Q [NFFT]`: the occupied bands of one wideband I/Q capture (2 channels, DECIM or P/Q x a
// supported rate), from one averaged power spectrum of NFFT (1280, 2560 or 5120; default 1280) bins over the whole file (ofdmrx_util_survey,
// ofdmrx_util_find_bands).  One line per band on stdout - centre Hz, width Hz, level dB over the floor - in
// ascending frequency: the centres `decode_stream --wideband DECIM c1,c2,... OUTROOT WIDE.wav` takes.  The floor goes to stderr.
// Exit status 0 (also when no band is found), 1 on argument, WAV or library errors.
// `survey --grid WIDE.wav DECIM [FLOOR_DB]`: the occupied slots of a grid capture (DECIM a power of two 2 .. 512; DESIGN.md section
// 4.21: ofdmrx_util_survey_grid in rows of 4096 output times, the per-slot maximum over the rows, ofdmrx_util_find_slots).  One line
// per slot on stdout - slot, centre Hz, level dB over the floor - in ascending order: the slots `decode_stream --grid DECIM k1,k2,...
// OUTROOT WIDE.wav` takes.  FLOOR_DB: an absolute floor, 10 log10 of the per-slot power re full scale; absent: the row's median.
// `survey --grid-ratio WIDE.wav P/Q [FLOOR_DB]`: the same for a grid capture at a ratio (DESIGN.md section 4.24:
// ofdmrx_util_survey_grid_ratio, ofdmrx_util_find_slots_ratio) - the capture's rate x Q / P must be a supported rate; the lines are
// those of --grid, the slots `decode_stream --grid P/Q k1,k2,... OUTROOT WIDE.wav` takes.  `--grid WIDE.wav P/Q` stays refused.
#include "survey_cli.h"
#include <cmath>
#include <cstdlib>

// `survey --grid WIDE.wav DECIM [FLOOR_DB]`, `survey --grid-ratio WIDE.wav P/Q [FLOOR_DB]`
static int run_grid(int argc, char **argv, bool at_ratio)
{
	const int decim = std::atoi(argv[3]);
	const Decimation ratio(argv[3]);
	double abs_floor = 0.0;
	if (!at_ratio && std::strchr(argv[3], '/')) {
		std::fprintf(stderr, "The grid survey at a ratio P/Q is not built under --grid, which takes a power of two 2 .. 512: use `survey --grid-ratio WIDE.wav P/Q [FLOOR_DB]` (DESIGN.md section 4.24).\n");
		return 1;
	}
	int32_t k_first = 0;
	size_t n_all = 0;
	if (at_ratio && (!ratio.ratio || ratio.p <= 0 || ratio.q <= 0 || ofdmrx_util_grid_ratio_slots(ratio.p, ratio.q, &k_first, &n_all) || (argc == 5 && !survey_floor_arg(argv[4], abs_floor)))) {
		std::fprintf(stderr, "A grid survey at a ratio takes P/Q (the spelling with '/') with, in lowest terms, Q 1 .. 16 and P 2 Q .. 512 with no prime factor other than 2, 3 and 5, and, optionally, a floor in dB re full scale.\n");
		return 1;
	}
	if (!at_ratio && (!grid_decim_valid(decim) || (argc == 5 && !survey_floor_arg(argv[4], abs_floor)))) {
		std::fprintf(stderr, "A grid survey takes a decimation that is a power of two 2 .. 512 and, optionally, a floor in dB re full scale.\n");
		return 1;
	}
	Wav w;
	if (!read_wav(argv[2], w) || w.frames == 0) {
		std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", argv[2]);
		return 1;
	}
	if (w.channels != 2) {
		std::fprintf(stderr, "A wideband capture is an analytic signal (two channels).\n");
		return 1;
	}
	const int rate = at_ratio ? ratio.rate_of(w.rate) : w.rate % decim ? 0 : w.rate / decim;
	if (rate != 8000 && rate != 16000 && rate != 44100 && rate != 48000) {
		std::fprintf(stderr, "Unsupported sample rate.\n");
		return 1;
	}
	if (ofdmrx_abi_version() != OFDMRX_ABI_VERSION || ofdmrx_abi_minor() < 9) {
		std::fprintf(stderr, "libofdmrx: ABI %d.%d, this program needs %d.9\n", ofdmrx_abi_version(), ofdmrx_abi_minor(), OFDMRX_ABI_VERSION);
		return 1;
	}
	ofdmrx_config cfg{};
	cfg.abi_version = OFDMRX_ABI_VERSION;
	cfg.sample_rate = rate;
	cfg.list_size = 8;
	cfg.chunk_frames = 1;
	cfg.descramble = 1;
	ofdmrx_handle *h = nullptr;
	const int r = ofdmrx_create(&cfg, &h);
	if (r) {
		std::fprintf(stderr, "ofdmrx_create: %s\n", ofdmrx_strerror(r));
		return 1;
	}
	std::vector<ofdmrx_slot> slots;
	double floor = 0.0;
	const bool ok = at_ratio ? survey_grid_ratio_capture(h, w, ratio.p, ratio.q, abs_floor, slots, floor) : survey_grid_capture(h, w, decim, abs_floor, slots, floor);
	ofdmrx_destroy(h);
	if (!ok)
		return 1;
	std::fprintf(stderr, "floor %.6g (%.2f dB), %zu slot%s\n", floor, floor > 0.0 ? 10.0 * std::log10(floor) : -999.0, slots.size(), slots.size() == 1 ? "" : "s");
	for (const ofdmrx_slot &s : slots)
		std::printf("%d %.2f %.2f\n", s.slot, s.centre_hz, (double)s.level_db);
	return 0;
}

int main(int argc, char **argv)
{
	if ((argc == 4 || argc == 5) && !std::strcmp(argv[1], "--grid"))
		return run_grid(argc, argv, false);
	if ((argc == 4 || argc == 5) && !std::strcmp(argv[1], "--grid-ratio"))
		return run_grid(argc, argv, true);
	if ((argc != 3 && argc != 4) || !std::strncmp(argv[1], "--", 2)) {
		std::fprintf(stderr, "usage: %s WIDE.wav DECIM|P/Q [NFFT]\n       %s --grid WIDE.wav DECIM [FLOOR_DB]\n       %s --grid-ratio WIDE.wav P/Q [FLOOR_DB]\n", argv[0], argv[0], argv[0]);
		return 1;
	}
	const Decimation decim(argv[2]);
	const int nfft = argc == 4 ? std::atoi(argv[3]) : 1280;
	if (!decim.valid() || (nfft != 1280 && nfft != 2560 && nfft != 5120)) {
		std::fprintf(stderr, "A survey takes a decimation of 2 .. 32 (a ratio P/Q: Q <= 16) and 1280, 2560 or 5120 bins.\n");
		return 1;
	}
	Wav w;
	if (!read_wav(argv[1], w) || w.frames == 0) {
		std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", argv[1]);
		return 1;
	}
	if (w.channels != 2) {
		std::fprintf(stderr, "A wideband capture is an analytic signal (two channels).\n");
		return 1;
	}
	const int rate = decim.rate_of(w.rate);
	if (!rate || (rate != 8000 && rate != 16000 && rate != 44100 && rate != 48000)) {
		std::fprintf(stderr, "Unsupported sample rate.\n");
		return 1;
	}
	if (ofdmrx_abi_version() != OFDMRX_ABI_VERSION || ofdmrx_abi_minor() < 9) {
		std::fprintf(stderr, "libofdmrx: ABI %d.%d, this program needs %d.9\n", ofdmrx_abi_version(), ofdmrx_abi_minor(), OFDMRX_ABI_VERSION);
		return 1;
	}
	ofdmrx_config cfg{};
	cfg.abi_version = OFDMRX_ABI_VERSION;
	cfg.sample_rate = rate;
	cfg.list_size = 8;
	cfg.chunk_frames = 1;
	cfg.descramble = 1;
	ofdmrx_handle *h = nullptr;
	const int r = ofdmrx_create(&cfg, &h);
	if (r) {
		std::fprintf(stderr, "ofdmrx_create: %s\n", ofdmrx_strerror(r));
		return 1;
	}
	std::vector<ofdmrx_band> bands;
	double floor = 0.0;
	const bool ok = survey_capture(h, w, nfft, bands, floor);
	ofdmrx_destroy(h);
	if (!ok)
		return 1;
	std::fprintf(stderr, "floor %.6g (%.2f dB), %zu band%s\n", floor, floor > 0.0 ? 10.0 * std::log10(floor) : -999.0, bands.size(), bands.size() == 1 ? "" : "s");
	for (const ofdmrx_band &b : bands)
		std::printf("%.2f %.2f %.2f\n", b.centre_hz, b.width_hz, (double)b.level_db);
	return 0;
}
