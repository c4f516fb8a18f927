// Host-side check of the LDS image of stft_tx1024_kernel (csrc/tx1024_lds_layout.h), the same constexpr functions the
// kernel indexes with: every table entry has one slot of its own, every 16-byte read is aligned and returns the two
// entries the kernel consumes, in order; exchange 1 delivers the permutation  consumer (lane t, register q)  <-  writer
// lane (t >> 4) + 4 q, register t & 15;  and the bank-conflict degree of every access under the LDS rules of the CDNA4
// notes (restated below as data).  Built (ASan + UBSan where available) and run by tests/test_tx1024_lds_layout.py.
// Prints one "degree NAME N" line per access kind and "ok"; exit code 0 = every check holds.
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "../../ssqueeze_rs_amd/csrc/tx1024_lds_layout.h"

using namespace ssq::tx1024;

static int fails = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      if (fails < 20) std::fprintf(stderr, "check failed (line %d): %s\n", __LINE__, #c); \
      ++fails;                                                         \
    }                                                                  \
  } while (0)

// ---- the LDS rules, as data: a wave64 access is served in fixed lane groups, one array cycle per group when no bank is
//      asked for two DIFFERENT addresses inside the group (identical addresses broadcast); masked-off lanes take no part.
struct Rule {
  const char* name;
  int bytes;                                   // per lane
  int banks;                                   // bank of byte address a = (a / 4) mod banks
  std::vector<std::vector<int>> groups;        // lanes of each group
};
static std::vector<int> span(std::initializer_list<std::pair<int, int>> rs, int shift = 0) {
  std::vector<int> v;
  for (auto r : rs)
    for (int l = r.first; l <= r.second; ++l) v.push_back(l + shift);
  return v;
}
static const Rule READ_B128 = {"ds_read_b128", 16, 64,
                               {span({{0, 3}, {12, 15}, {20, 27}}), span({{4, 11}, {16, 19}, {28, 31}}),
                                span({{0, 3}, {12, 15}, {20, 27}}, 32), span({{4, 11}, {16, 19}, {28, 31}}, 32)}};
static const Rule WRITE_B64 = {"ds_write_b64 (each half of ds_write2_b64)", 8, 32,
                               {span({{0, 15}}), span({{16, 31}}), span({{32, 47}}), span({{48, 63}})}};

// worst number of distinct addresses that meet on one bank inside one lane group (1 = conflict-free);
// addr[lane] = byte address, < 0 = lane masked off
static int degree(const Rule& rule, const std::vector<long>& addr) {
  int worst = 0;
  for (const auto& g : rule.groups) {
    std::vector<std::set<long>> on_bank((size_t)rule.banks);
    for (int lane : g) {
      if (addr[(size_t)lane] < 0) continue;
      for (int d = 0; d < rule.bytes / 4; ++d) {
        const long dw = addr[(size_t)lane] / 4 + d;
        on_bank[(size_t)(dw % rule.banks)].insert(dw);
      }
    }
    for (const auto& s : on_bank) worst = std::max(worst, (int)s.size());
  }
  return worst;
}

// a table as the kernel's prologue fills it: tag[slot] = which entry lives there, -1 = nothing
struct Table {
  std::vector<int> tag;
  explicit Table(int elems) : tag((size_t)elems, -1) {}
  void put(int slot, int what) {
    CHECK(slot >= 0 && slot < (int)tag.size());
    if (slot < 0 || slot >= (int)tag.size()) return;
    CHECK(tag[(size_t)slot] == -1);                          // exactly one entry per slot
    tag[(size_t)slot] = what;
  }
  // the 16-byte read at element index `row`: aligned, in bounds, returns (first, second)
  void pair(int row, int first, int second) const {
    CHECK(row % 2 == 0);
    CHECK(row >= 0 && row + 1 < (int)tag.size());
    if (row < 0 || row + 1 >= (int)tag.size()) return;
    CHECK(tag.data()[row] == first);
    CHECK(tag.data()[row + 1] == second);
  }
};

int main() {
  int deg_win = 0, deg_tw1 = 0, deg_tw2 = 0, deg_st = 0, deg_ld = 0;
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
  CHECK(EXCH_OFF % 16 == 0 && (EXCH_ELEMS * 8) % 16 == 0 && WIN_OFF % 16 == 0 && TW1_OFF % 16 == 0 && TW2_OFF % 16 == 0);
  CHECK(EXCH_OFF >= TILE_BYTES && WIN_OFF >= EXCH_OFF + W * EXCH_ELEMS * 8 && TW1_OFF >= WIN_OFF + WIN_ELEMS * 8 &&
        TW2_OFF >= TW1_OFF + TW1_ELEMS * 8 && LDS_BYTES >= TW2_OFF + TW2_ELEMS * 8);

  // ---- window: element e = t + 64 q; lane t reads pair j = (q = 2 j, 2 j + 1)
  {
    Table win(WIN_ELEMS);
    for (int e = 0; e < N; ++e) win.put(win_slot(e), e);
    for (int s = 0; s < WIN_ELEMS; ++s) CHECK(win.tag[(size_t)s] == win_elem(s));     // the prologue fills by slot
    for (int j = 0; j < 8; ++j) {
      std::vector<long> addr(64);
      for (int t = 0; t < L; ++t) {
        win.pair(win_row(t, j), t + L * (2 * j), t + L * (2 * j + 1));
        addr[(size_t)t] = WIN_OFF + 8L * win_row(t, j);
      }
      deg_win = std::max(deg_win, degree(READ_B128, addr));
    }
  }
  // ---- pass-1 twiddles: entry (k, m) = W_256^(k m), m = 1..15 (+ filler "m = 16"); lane t reads pair i = (2 i + 1, 2 i + 2)
  {
    Table tw1(TW1_ELEMS);
    for (int k = 0; k < 16; ++k)
      for (int m = 1; m <= 16; ++m) tw1.put(tw1_slot(k, m), 16 * k + (m & 15) + (m == 16 ? 1000 : 0));
    for (int s = 0; s < TW1_ELEMS; ++s) {                                               // the prologue fills by slot
      const int k = tw1_k(s), m = tw1_m(s);
      CHECK(k >= 0 && k < 16 && m >= 0 && m < 16);
      if (m > 0) CHECK(tw1.tag[(size_t)s] == 16 * k + m);
      else CHECK(tw1.tag[(size_t)s] == -1 || tw1.tag[(size_t)s] == 16 * k + 1000);     // pad or filler: W^0
    }
    for (int i = 0; i < 8; ++i) {
      std::vector<long> addr(64);
      for (int t = 0; t < L; ++t) {
        const int k = t & 15;
        tw1.pair(tw1_row(k, i), 16 * k + 2 * i + 1, i < 7 ? 16 * k + 2 * i + 2 : 16 * k + 1000);
        addr[(size_t)t] = TW1_OFF + 8L * tw1_row(k, i);
      }
      deg_tw1 = std::max(deg_tw1, degree(READ_B128, addr));
    }
  }
  // ---- pass-2 twiddles: entry (t, b, m) = W_1024^((t + 64 b) m); lane t consumes e = 3 b + (m - 1) in order, pair i = e >> 1
  {
    Table tw2(TW2_ELEMS);
    for (int t = 0; t < L; ++t)
      for (int b = 0; b < 4; ++b)
        for (int m = 1; m <= 3; ++m) tw2.put(tw2_slot(t, b, m), (t + L * b) * 4 + m);
    for (int s = 0; s < TW2_ELEMS; ++s) CHECK(tw2.tag[(size_t)s] == tw2_j(s) * 4 + tw2_m(s));   // the prologue fills by slot
    for (int i = 0; i < 6; ++i) {
      std::vector<long> addr(64);
      for (int t = 0; t < L; ++t) {
        const int e0 = 2 * i, e1 = 2 * i + 1;
        tw2.pair(tw2_row(t, i), (t + L * (e0 / 3)) * 4 + e0 % 3 + 1, (t + L * (e1 / 3)) * 4 + e1 % 3 + 1);
        addr[(size_t)t] = TW2_OFF + 8L * tw2_row(t, i);
      }
      deg_tw2 = std::max(deg_tw2, degree(READ_B128, addr));
    }
  }
  // ---- exchange 1, every wave's row, both phases: in phase ph writer lane a stores registers 8 ph + u, u < 8; the lanes
  //      with ((t >> 3) & 1) == ph read all 16 of their new registers q: writer (t >> 4) + 4 q, register t & 15
  for (int wave = 0; wave < W; ++wave)
    for (int ph = 0; ph < 2; ++ph) {
      const long row0 = EXCH_OFF + 8L * EXCH_ELEMS * wave;
      Table row(EXCH_ELEMS);
      for (int u = 0; u < 8; ++u) {
        std::vector<long> addr(64);
        for (int a = 0; a < L; ++a) {
          const int slot = exch_store_base(a) + exch_val(u);
          CHECK(slot < EXCH_USED);
          row.put(slot, 16 * a + 8 * ph + u);
          addr[(size_t)a] = row0 + 8L * slot;
        }
        deg_st = std::max(deg_st, degree(WRITE_B64, addr));
      }
      std::vector<int> times_read((size_t)EXCH_ELEMS, 0);
      for (int g = 0; g < 8; ++g) {
        std::vector<long> addr(64, -1);
        for (int t = 0; t < L; ++t) {
          if (((t >> 3) & 1) != ph) continue;
          const int at = exch_load_base(t) + exch_load_off(g);
          row.pair(at, 16 * ((t >> 4) + 4 * (2 * g)) + (t & 15), 16 * ((t >> 4) + 4 * (2 * g + 1)) + (t & 15));
          if (at >= 0 && at + 1 < EXCH_ELEMS) ++times_read[(size_t)at], ++times_read[(size_t)at + 1];
          addr[(size_t)t] = row0 + 8L * at;
        }
        deg_ld = std::max(deg_ld, degree(READ_B128, addr));
      }
      for (int s = 0; s < EXCH_ELEMS; ++s) CHECK(times_read[(size_t)s] == (row.tag[(size_t)s] >= 0 ? 1 : 0));
    }

  std::printf("degree window %d\ndegree tw1 %d\ndegree tw2 %d\ndegree exch_store %d\ndegree exch_load %d\n", deg_win,
              deg_tw1, deg_tw2, deg_st, deg_ld);
  std::printf("lds_bytes %d\n", LDS_BYTES);
  std::printf(fails ? "FAILED\n" : "ok\n");
  return fails ? 1 : 0;
}
