// Host test of chunk_walk.h's index plan and walker (no HIP): every thread of a simulated block walks a row, for
// every element size, offset from a 16-byte boundary, row length, thread stride and value of the "vector allowed"
// flag.  Build: g++ -std=c++17 -I csrc/kernels csrc/kernels/tests/chunk_walk_test.cpp
#include <stdio.h>

#include <vector>

#include "chunk_walk.h"

using namespace dtm;

static int failures = 0;
#define CHECK(cond, ...)                                                              \
  do {                                                                                \
    if (!(cond) && ++failures <= 20) printf("FAIL %s: ", #cond), printf(__VA_ARGS__), printf("\n"); \
  } while (0)

template <int STRIDE, int ELEM>
static void check_rows() {
  constexpr int VEC = 16 / ELEM;
  for (int off = 0; off < 16; off += ELEM) {
    const uintptr_t addr = 0x10000u + (uintptr_t)off;  // never dereferenced
    for (int len = 0; len <= 70; ++len) {
      for (int ok = 0; ok < 2; ++ok) {
        const WalkPlan w = walk_plan(ELEM, addr, len, ok != 0);
        const int h16 = head_elems(addr, ELEM);
        CHECK((addr + (uintptr_t)h16 * ELEM) % 16 == 0 && h16 < VEC, "head_elems %d off %d", h16, off);
        CHECK(w.len == len, "len %d", w.len);
        if (ok) {
          CHECK(w.head == (h16 < len ? h16 : len), "head %d (len %d, off %d): a row shorter than its head", w.head,
                len, off);
          CHECK(w.nvec >= 0 && w.tail0 == w.head + w.nvec * VEC && w.tail0 <= len && len - w.tail0 < VEC,
                "plan {%d, %d, %d} len %d", w.head, w.nvec, w.tail0, len);
        } else {
          CHECK(w.head == 0 && w.nvec == 0 && w.tail0 == 0, "scalar plan {%d, %d, %d}", w.head, w.nvec, w.tail0);
        }
        std::vector<int> seen(len, 0);
        for (int tid = 0; tid < STRIDE; ++tid) {
          int last = -1, phase = 0;  // phase 0: head, 1: body, 2: tail
          walk<STRIDE, VEC>(
              w, tid,
              [&](int i) {
                CHECK(i >= 0 && i < len, "scalar index %d of %d", i, len);
                if (i < 0 || i >= len) return;
                const int ph = i < w.head ? 0 : 2;
                CHECK(i < w.head || i >= w.tail0, "scalar index %d inside the body", i);
                CHECK(ph >= phase && i > last, "thread %d: scalar %d after %d (phase %d -> %d)", tid, i, last, phase, ph);
                phase = ph;
                last = i;
                ++seen[i];
              },
              [&](int g, int base) {
                CHECK(ok, "a vector group without the flag");
                CHECK(base == w.head + g * VEC && g >= 0 && g < w.nvec, "group %d base %d", g, base);
                CHECK((addr + (uintptr_t)base * ELEM) % 16 == 0, "group at element %d is not on a 16-byte boundary", base);
                CHECK(base >= 0 && base + VEC <= len, "group [%d, %d) outside the row of %d", base, base + VEC, len);
                CHECK(phase <= 1 && base > last, "thread %d: group at %d after %d (phase %d)", tid, base, last, phase);
                phase = 1;
                if (base < 0 || base + VEC > len) return;
                for (int e = 0; e < VEC; ++e) ++seen[base + e];
                last = base + VEC - 1;
              });
        }
        for (int i = 0; i < len; ++i)
          CHECK(seen[i] == 1, "element %d of %d visited %d times (elem %d, off %d, stride %d, flag %d)", i, len,
                seen[i], ELEM, off, STRIDE, ok);
      }
    }
  }
}

int main() {
  check_rows<64, 2>();
  check_rows<64, 4>();
  check_rows<256, 2>();
  check_rows<256, 4>();

  // chunk_len: whole rows, the last row, a row at or past the end (a tensor whose length was set to 0)
  CHECK(chunk_len(8192, 0, 8192) == 8192, "whole");
  CHECK(chunk_len(8193, 8192, 8192) == 1, "last");
  CHECK(chunk_len(20000, 8192, 8192) == 8192, "middle");
  CHECK(chunk_len(0, 8192, 8192) == 0 && chunk_len(5, 5, 8192) == 0, "past the end");
  CHECK(chunk_len((1L << 33) + 7, 1L << 33, 32768) == 7, "64-bit start");

  // same16 / copy8_ok on plain addresses
  char* const b = (char*)(uintptr_t)0x20000u;
  CHECK(same16(b + 4, b + 20, b + 36) && !same16(b + 4, b + 20, b + 40) && same16(b), "same16");
  // fp32 array 1 element past a boundary: head 3 elements, so the bf16 copy must sit 6 bytes before an 8-byte one
  CHECK(copy8_ok(nullptr, 0x20004u) && copy8_ok(b + 2, 0x20004u) && !copy8_ok(b + 4, 0x20004u), "copy8_ok");
  CHECK(copy8_ok(b, 0x20000u) && !copy8_ok(b + 2, 0x20000u), "copy8_ok aligned");

  if (failures) {
    printf("chunk_walk test: %d failure(s)\n", failures);
    return 1;
  }
  printf("chunk_walk test OK\n");
  return 0;
}
