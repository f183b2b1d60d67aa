// tx_band.h -- the transmitter's band check (encode.cc:363-392), one copy for the C ABI (api_tx.cpp) and the `encode` CLI
// (encode_main.cpp).  Plain host C++: no HIP, nothing from the library.
#pragma once

// encode.cc:363-387; 0 for a mode outside 6..13
static inline int tx_band_width(int oper_mode)
{
	static const int bw[14] = { 0, 0, 0, 0, 0, 0, 2700, 2500, 2500, 2250, 3200, 2400, 2400, 1600 };
	return oper_mode >= 6 && oper_mode <= 13 ? bw[oper_mode] : 0;
}

// encode.cc:389 with its integer halves: false is "Unsupported frequency offset." - the band has to fit between the spectrum's edges
// (one channel: above 0 Hz); outside, the carriers would fold round Nyquist
static inline bool tx_offset_in_band(int rate, int oper_mode, int channels, int freq_off)
{
	const int band_width = tx_band_width(oper_mode);
	return !((channels == 1 && freq_off < band_width / 2) || freq_off < band_width / 2 - rate / 2 || freq_off > rate / 2 - band_width / 2);
}
