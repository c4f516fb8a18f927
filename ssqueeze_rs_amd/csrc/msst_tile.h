// msst_tile.h -- the LDS tile of the two multisynchrosqueezing walk kernels, stft_msst.hip (msst_walk_kernel)
// and cwt_msst.hip (cwt_msst_walk_kernel): a workgroup owns C consecutive columns of one signal and all
// rows, one 16-bit word per element.
#pragma once

namespace ssq {

constexpr int kWalkThreads = 512;
// 16-bit words of a tile: C = 2^15 / (n_fft / 2) columns, 16 (n_fft 4096) .. 256 (n_fft <= 256), of n_fft/2 + 1 rows make
// 2^15 + C words, at most 66048 bytes: two workgroups share a CU's 160 KB of LDS.
constexpr int kWalkTileWords = 129 * 256;
constexpr int kWalkMinLogCols = 4, kWalkMaxLogCols = 8;
constexpr int kWalkMaxRows = 2049;
constexpr int kWalkMaxIter = 64;
constexpr unsigned kWalkNoMap = 0xffffu;

// log2 of the tile width for `n_rows` rows (1 .. kWalkMaxRows): the widest tile of 16 .. 256 columns that fits
inline int walk_log_cols(int n_rows) {
  int lc = kWalkMaxLogCols;
  while (lc > kWalkMinLogCols && (n_rows << lc) > kWalkTileWords) --lc;
  return lc;
}

}  // namespace ssq
