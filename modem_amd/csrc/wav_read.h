// wav_read.h -- the WAV reader of the decode CLIs (decode_main.cpp, decode_stream_main.cpp): DSP::ReadWAV's contract
#pragma once
#include "../../include/ofdmrx.h"
#include <cstdio>
#include <cstring>
#include <vector>

static uint32_t rd32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

struct Wav { int rate = 0, bits = 0, channels = 0, fmt = -1; size_t frames = 0; std::vector<uint8_t> pcm; };

// DSP::ReadWAV contract (decode.cc:576-578,590): RIFF/WAVE PCM, 8-bit unsigned, 16/24/32-bit signed LE
static bool read_wav(const char *name, Wav &w)
{
	FILE *f = std::fopen(name, "rb");
	if (!f)
		return false;
	std::vector<uint8_t> buf;
	uint8_t tmp[65536];
	size_t n;
	while ((n = std::fread(tmp, 1, sizeof(tmp), f)) > 0)
		buf.insert(buf.end(), tmp, tmp + n);
	std::fclose(f);
	if (buf.size() < 12 || std::memcmp(buf.data(), "RIFF", 4) || std::memcmp(buf.data() + 8, "WAVE", 4))
		return false;
	size_t pos = 12;
	bool have_fmt = false;
	while (pos + 8 <= buf.size()) {
		uint32_t sz = rd32(&buf[pos + 4]);
		const uint8_t *body = &buf[pos + 8];
		if (!std::memcmp(&buf[pos], "fmt ", 4) && sz >= 16) {
			w.channels = rd16(body + 2);
			w.rate = (int)rd32(body + 4);
			w.bits = rd16(body + 14);
			have_fmt = true;
		} else if (!std::memcmp(&buf[pos], "data", 4) && have_fmt) {
			size_t avail = buf.size() - (pos + 8);
			if (sz > avail)
				sz = (uint32_t)avail;
			int bytes = w.bits / 8;
			if (bytes < 1 || bytes > 4 || w.channels < 1)
				return false;
			w.frames = sz / (size_t)(bytes * w.channels);
			size_t cnt = w.frames * (size_t)w.channels;
			if (bytes == 1) {
				w.fmt = OFDMRX_FMT_U8;
				w.pcm.assign(body, body + cnt);
			} else if (bytes == 2) {
				w.fmt = OFDMRX_FMT_S16;
				w.pcm.assign(body, body + 2 * cnt);   // little endian host
			} else {
				w.fmt = OFDMRX_FMT_F32;
				w.pcm.resize(4 * cnt);
				float *d = (float *)w.pcm.data();
				float factor = (float)((1u << (w.bits - 1)) - 1);
				for (size_t i = 0; i < cnt; ++i) {
					int32_t v = 0;
					for (int b = 0; b < bytes; ++b)
						v |= (int32_t)((uint32_t)body[bytes * i + b] << (8 * b + 8 * (4 - bytes)));
					v >>= 8 * (4 - bytes);
					d[i] = (float)v / factor;
				}
			}
			return true;
		}
		pos += 8 + (size_t)sz + (sz & 1);
	}
	return false;
}
