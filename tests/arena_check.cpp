// Stand-alone check of the workspace arena (newsreclib_amd/csrc/nrl_arena.h): a few hundred pseudo-random layouts, each run once
// measuring and once carving, as every entry point of the library does.  Built and run by tests/test_workspace_host.py:
//   c++ -std=c++17 -I newsreclib_amd/csrc tests/arena_check.cpp -o arena_check && ./arena_check
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "nrl_arena.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;   // fixed seed
uint64_t rnd() {                               // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Take {
  int type;  // 0 float, 1 uint16_t, 2 unsigned char, 3 double, 4 int32_t
  size_t lead, count, align;
};
const size_t kSize[5] = {sizeof(float), sizeof(uint16_t), 1, sizeof(double), sizeof(int32_t)};

struct Region {
  uintptr_t begin, end, ptr;   // the reserved bytes and the pointer handed out (begin + lead elements)
};

// one take of the sequence on `a`; null from a measuring arena
void* run(nrl::Arena& a, const Take& t) {
  switch (t.type) {
    case 0: return t.lead ? a.take_after<float>(t.lead, t.count, t.align) : a.take<float>(t.count, t.align);
    case 1: return t.lead ? a.take_after<uint16_t>(t.lead, t.count, t.align) : a.take<uint16_t>(t.count, t.align);
    case 2: return t.lead ? a.take_after<unsigned char>(t.lead, t.count, t.align) : a.take<unsigned char>(t.count, t.align);
    case 3: return t.lead ? a.take_after<double>(t.lead, t.count, t.align) : a.take<double>(t.count, t.align);
    default: return t.lead ? a.take_after<int32_t>(t.lead, t.count, t.align) : a.take<int32_t>(t.count, t.align);
  }
}

int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (failures++ < 20) {                  \
        fprintf(stderr, "FAIL %s: ", #cond); \
        fprintf(stderr, __VA_ARGS__);         \
        fprintf(stderr, "\n");                \
      }                                       \
    }                                         \
  } while (0)

}  // namespace

int main() {
  const size_t aligns[] = {8, 16, 64, 256, 256, 256, 1024};
  int sequences = 0;
  size_t takes = 0;
  for (int seq = 0; seq < 400; ++seq) {
    std::vector<Take> plan;
    const int n = 1 + (int)(rnd() % 24);
    for (int i = 0; i < n; ++i) {
      Take t;
      t.type = (int)(rnd() % 5);
      t.align = aligns[rnd() % 7];
      const uint64_t kind = rnd() % 8;
      t.count = kind == 0 ? 0 : (kind == 1 ? 1 : (kind < 6 ? rnd() % 700 : rnd() % 70000));   // zero-sized takes included
      t.lead = (rnd() % 4 == 0 && t.count > 0) ? rnd() % (t.count + 1) : 0;                    // leading slack (up to the whole region)
      plan.push_back(t);
    }
    // measuring: no base, no pointer may come back
    nrl::Arena m;
    for (const Take& t : plan) CHECK(run(m, t) == nullptr, "sequence %d: a measuring take returned a pointer", seq);
    const size_t total = m.bytes();
    // carving, on a 1024-byte aligned base with a canary band behind the measured total
    std::vector<unsigned char> buf(total + 1024 + 64, 0xA5);
    unsigned char* base = reinterpret_cast<unsigned char*>(((uintptr_t)buf.data() + 1023) & ~(uintptr_t)1023);
    nrl::Arena c(base);
    std::vector<Region> regions;
    for (const Take& t : plan) {
      const size_t before = c.bytes();
      unsigned char* p = static_cast<unsigned char*>(run(c, t));
      Region r;
      r.ptr = (uintptr_t)p;
      r.begin = r.ptr - t.lead * kSize[t.type];
      r.end = r.begin + t.count * kSize[t.type];
      CHECK(p != nullptr, "sequence %d: a carving take returned null", seq);
      CHECK((r.begin - (uintptr_t)base) % t.align == 0, "sequence %d: region at +%zu not aligned to %zu", seq, (size_t)(r.begin - (uintptr_t)base), t.align);
      CHECK(r.begin % kSize[t.type] == 0, "sequence %d: region misaligned for its element type", seq);
      CHECK(r.begin >= (uintptr_t)base + before, "sequence %d: region starts inside what was already used", seq);
      CHECK(r.end <= (uintptr_t)base + c.bytes(), "sequence %d: region ends past the used bytes", seq);
      CHECK(r.begin >= (uintptr_t)base && r.end <= (uintptr_t)base + total, "sequence %d: region outside [base, base + total)", seq);
      CHECK(c.bytes() % t.align == 0, "sequence %d: used bytes not padded to the alignment", seq);
      for (uintptr_t q = r.begin; q < r.end; ++q) *reinterpret_cast<unsigned char*>(q) = (unsigned char)regions.size();
      regions.push_back(r);
      ++takes;
    }
    CHECK(c.bytes() == total, "sequence %d: measured %zu bytes, carved %zu", seq, total, c.bytes());
    for (size_t i = 0; i < regions.size(); ++i) {
      for (size_t j = i + 1; j < regions.size(); ++j)
        CHECK(regions[i].end <= regions[j].begin || regions[j].end <= regions[i].begin || regions[i].begin == regions[i].end ||
                  regions[j].begin == regions[j].end, "sequence %d: regions %zu and %zu overlap", seq, i, j);
      // every byte still carries its own region's mark: no later region wrote into it
      for (uintptr_t q = regions[i].begin; q < regions[i].end; ++q)
        if (*reinterpret_cast<unsigned char*>(q) != (unsigned char)i) {
          CHECK(false, "sequence %d: region %zu was overwritten", seq, i);
          break;
        }
    }
    for (size_t k = 0; k < 64; ++k) CHECK(base[total + k] == 0xA5, "sequence %d: byte %zu past the total was written", seq, k);
    ++sequences;
  }
  if (failures != 0) {
    fprintf(stderr, "arena_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("arena_check OK: %d sequences, %zu takes\n", sequences, takes);
  return 0;
}
