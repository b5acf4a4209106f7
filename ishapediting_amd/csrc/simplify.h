// Quadric vertex clustering (csrc/simplify.hip; the rule: include/ishap.h, "Mesh simplification").  Constants the kernels, the
// scratch layout and the host checks share.  Internal: C++ linkage, no C ABI.
#pragma once
#include "common.h"
#include "scan.h"

constexpr long long SIMPLIFY_MAX_CELLS = 1ll << 30;     // gx gy gz: a cell id and a cluster id fit an int, the bitmap 128 MiB
constexpr int SIMPLIFY_ROW = 16;                        // u64 slots of a cluster's row: 128 bytes, one atomic segment
// slots: 0 vertex count, 1..3 sum rint(p 2^32), 4 lowest vertex index (min), 5..14 the quadric (A00 A01 A02 A11 A12 A22 b0 b1 b2 c,
// each rint(value 2^36)), 15 sum ceil(w) (the overflow guard)
constexpr int SIMPLIFY_SLOT_COUNT = 0, SIMPLIFY_SLOT_P = 1, SIMPLIFY_SLOT_MIN = 4, SIMPLIFY_SLOT_Q = 5, SIMPLIFY_SLOT_GUARD = 15;
constexpr double SIMPLIFY_P_SCALE = 4294967296.0;       // 2^32
constexpr double SIMPLIFY_Q_SCALE = 68719476736.0;      // 2^36
constexpr long long SIMPLIFY_GUARD = 1ll << 26;         // a referenced cluster whose sum ceil(w) reaches this fails the call
constexpr unsigned SIMPLIFY_EMPTY = 0xffffffffu;        // an empty slot of the triangle table
constexpr int SIMPLIFY_COUNTERS = 64;                  // words the count of non-degenerate triangles is gathered in (ints 64..127 of the header)
constexpr int SIMPLIFY_HDR_BYTES = 512;
enum { SIMPLIFY_QUADRIC = 0, SIMPLIFY_AVERAGE = 1 };
enum { SIMPLIFY_STATUS_OVERFLOW = 1 };

struct SimplifyGrid {
  double lo[3], h;
  int g[3];
};

// device scratch of one count / emit pair (each buffer 256-byte aligned; the header is at offset 0)
struct SimplifyLayout {
  long long words;      // 32-bit words of the cell bitmap
  long long cmax;       // most clusters there can be: min(nverts, cells)
  long long table;      // slots of the triangle table: a power of two >= max(2 ntris, 64)
  int *hdr, *vcluster;  // hdr: int[0] clusters, int[1] non-degenerate triangles, int[64..127] partial counts
  unsigned *bitmap, *prefix, *ref, *tab, *flag, *totals;
  unsigned long long* rows;
  long long bytes;
};
inline SimplifyLayout simplify_layout(void* base, long long nverts, long long ntris, long long cells) {
  Carve c{(char*)base};
  SimplifyLayout L;
  L.words = (cells + 31) / 32;
  L.cmax = nverts < cells ? nverts : cells;
  L.table = 64;
  while (L.table < 2 * ntris) L.table <<= 1;
  long long longest = L.words > L.cmax + 1 ? L.words : L.cmax + 1;
  if (ntris + 1 > longest) longest = ntris + 1;
  L.hdr = c.take<int>(SIMPLIFY_HDR_BYTES / sizeof(int));
  L.bitmap = c.take<unsigned>(L.words);
  L.prefix = c.take<unsigned>(L.words);
  L.vcluster = c.take<int>(nverts);
  L.rows = c.take<unsigned long long>(SIMPLIFY_ROW * L.cmax);
  L.ref = c.take<unsigned>(L.cmax + 1);
  L.tab = c.take<unsigned>(L.table);
  L.flag = c.take<unsigned>(ntris + 1);
  L.totals = c.take<unsigned>(scan_u32_blocks(longest) + 1);
  L.bytes = c.total();
  return L;
}
