// tx1024_lds_layout.h -- where stft_tx1024_kernel keeps its window, its twiddles and its exchange-1 row in LDS.
//
// Plain constexpr index arithmetic, no HIP: the kernel (stft_fused.hip) and the host-side checker
// (tests/helpers/tx1024_lds_layout_check.cpp) call the same functions.  Every index counts 8-byte complex elements from
// the start of its own table; every table starts 16-byte aligned.
//
// The layouts exist so that the two elements a lane consumes together are ADJACENT and 16-byte aligned: one ds_read_b128
// (4 LDS-array cycles per wave) fetches what took a two-address ds_read2_b64 / ds_read2st64_b64 (8 cycles).  The pitches
// are chosen for the 16-lane groups and the (byte address / 4) mod 64 bank rule of that instruction.
#pragma once

namespace ssq {
namespace tx1024 {

constexpr int N = 1024, L = 64;

// ---- window: [j][t][2], j < 8, t < 64 -- the entries of elements t + 128 j and t + 128 j + 64 are adjacent.
//      Lane t reads row (j, t) = elements q = 2 j and 2 j + 1 of its 16; consecutive lanes are contiguous.
constexpr int WIN_ELEMS = N;
constexpr int win_row(int t, int j) { return 2 * (L * j + t); }
constexpr int win_slot(int e) { return win_row(e & (L - 1), e >> 7) + ((e >> 6) & 1); }
constexpr int win_elem(int s) { return ((s >> 1) & (L - 1)) + L * (2 * (s >> 7) + (s & 1)); }     // inverse: slot -> element

// ---- pass-1 twiddles W_256^(k m): [k][m - 1], k = t & 15, m = 1..15, then one filler (the prologue stores
//      W^0 there, "m = 16") that completes the last pair.  m = 0 needs no entry.  Row pitch 18 elements = 36 dwords: 36 k mod 64
//      puts the 16 rows on the 16 distinct 4-dword bank slots; lanes with equal k read one address (broadcast).
//      Lane reads pair i = entries m = 2 i + 1, 2 i + 2.  (With the filler in FRONT, m = 0, the compiler narrows the
//      first read to its used half and re-pairs the whole row from there, 8 bytes off: seven two-address reads again.)
constexpr int TW1_PITCH = 18;
constexpr int TW1_ELEMS = 16 * TW1_PITCH;
constexpr int tw1_slot(int k, int m) { return TW1_PITCH * k + m - 1; }
constexpr int tw1_row(int k, int i) { return tw1_slot(k, 2 * i + 1); }
constexpr int tw1_k(int s) { return s / TW1_PITCH; }                                               // inverse: slot -> (k, m);
constexpr int tw1_m(int s) { return s % TW1_PITCH < 15 ? s % TW1_PITCH + 1 : 0; }                  // filler and pads: m = 0

// ---- pass-2 twiddles W_1024^((t + 64 b) m): lane t consumes 12 entries e = 3 b + (m - 1) (b-major, m = 1..3, the
//      order of the butterflies) as pairs i = e >> 1.  Layout [i][t][2], the window's: consecutive lanes are contiguous
//      (no conflicts, no padding), and the lane's byte offset 16 t is the window's, so both tables are read off ONE
//      address register.  (A per-lane row [t][12] at pitch 14 is conflict-free as well, but costs 1 KiB of padding and
//      an address register of its own: three more spilled dwords in the tile loop.)
constexpr int TW2_ELEMS = 3 * 256;
constexpr int tw2_row(int t, int i) { return 2 * (L * i + t); }
constexpr int tw2_slot(int t, int b, int m) { return tw2_row(t, (3 * b + m - 1) >> 1) + ((3 * b + m - 1) & 1); }
constexpr int tw2_e(int s) { return 2 * (s >> 7) + (s & 1); }                                      // inverse: slot -> entry e,
constexpr int tw2_j(int s) { return ((s >> 1) & (L - 1)) + L * (tw2_e(s) / 3); }                   // j = t + 64 b
constexpr int tw2_m(int s) { return tw2_e(s) % 3 + 1; }

constexpr int TAB_ELEMS = WIN_ELEMS + TW1_ELEMS + TW2_ELEMS;

// ---- exchange 1, one half-frame row per wave.  In a phase every lane a (the writer) stores its 8 values u = 0..7; the
//      consumer lane t (r = t >> 4, value u = t & 7) reads the writers a = r + 4 q, q = 0..15, as 8 pairs g = q >> 1.
//      Writer a's value u lies at  block(a & 3, a >> 3) + val(u) + ((a >> 2) & 1):
//        * the values of writers a and a + 4 (q = 2 g, 2 g + 1) are adjacent and 16-byte aligned (block, val even);
//        * val(u) = 4 (u & 3) + 2 (u >> 2) is lane-independent: the 8 stores keep immediate offsets;
//        * block mod 16 = 4 r + 2 (g & 1): with the writer's q & 1 the 16 lanes of a store group fall on the 16
//          distinct 2-dword bank pairs of the 32 store banks;
//        * a 16-lane load group holds, under a phase's half exec mask, values u & 3 = 0..3 of two rows r, one with
//          u < 4 and one with u >= 4: their 4-dword bank slots are block / 2 + {0, 2, 4, 6} and block' / 2 + {1, 3, 5, 7}
//          with block' - block = 132 -- an even slot distance, so the two sets never meet.  (With val(u) = 2 u the sets
//          are runs of four slots at distance 2 mod 8: a 2-way conflict in every other group.)
constexpr int EXCH_ELEMS = 576;                       // per wave; the layout fills 526
constexpr int exch_block(int r, int g) { return 66 * (2 * r + (g & 1)) + 16 * (g >> 1); }
constexpr int exch_val(int u) { return 4 * (u & 3) + 2 * (u >> 2); }
constexpr int exch_store_base(int a) { return exch_block(a & 3, a >> 3) + ((a >> 2) & 1); }     // + exch_val(u)
constexpr int exch_load_base(int t) { return exch_block(t >> 4, 0) + exch_val(t & 7); }         // + exch_load_off(g)
constexpr int exch_load_off(int g) { return exch_block(0, g); }
constexpr int EXCH_USED = exch_block(3, 7) + 16;

static_assert(EXCH_USED <= EXCH_ELEMS, "exchange row");
static_assert(exch_block(3, 5) == exch_block(3, 0) + exch_load_off(5), "block index is additive in (r, g)");

// ---- the kernel's whole LDS image, in bytes: scatter tile [NF][PITCH] 64-bit cells + F column scales | W exchange rows
//      | window | pass-1 twiddles | pass-2 twiddles
constexpr int NF = N / 2 + 1, F = 16, PITCH = F + 1, W = 16;
constexpr int TILE_BYTES = (((2 * NF * PITCH + F) * 4 + 15) / 16) * 16;
constexpr int EXCH_OFF = TILE_BYTES;
constexpr int WIN_OFF = EXCH_OFF + W * EXCH_ELEMS * 8;
constexpr int TW1_OFF = WIN_OFF + WIN_ELEMS * 8;
constexpr int TW2_OFF = TW1_OFF + TW1_ELEMS * 8;
constexpr int LDS_BYTES = TW2_OFF + TW2_ELEMS * 8;
static_assert(EXCH_OFF % 16 == 0 && (EXCH_ELEMS * 8) % 16 == 0 && WIN_OFF % 16 == 0 && TW1_OFF % 16 == 0 && TW2_OFF % 16 == 0,
              "16-byte reads: every table and every wave's exchange row starts 16-byte aligned");
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");

}  // namespace tx1024
}  // namespace ssq
