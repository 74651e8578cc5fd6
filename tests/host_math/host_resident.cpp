// csrc/resident_kernels.hip compiled as HOST code (hip_shim/) and run lane by lane against a plain per-graph memcpy
// collate: a stand-alone program for -fsanitize=address,undefined.  Every buffer is an exact-size heap allocation, so a
// load past a resident tensor or a store past a destination is a sanitizer report; the bytes in front of a misaligned
// destination are a canary; uint4 / longlong2 are alignas(16), so a 16-byte access that is not aligned is one too.
// Sources and destinations take every 4-byte (8-byte for the int64 kinds) offset from a 16-byte boundary at random.
#include "../../caster-dta_amd/csrc/resident_kernels.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
using std::vector;

static std::mt19937_64 rng(7);

struct Buf {  // payload of exactly `bytes`, starting `lead` bytes behind a 16-byte aligned address
  char *raw, *p;
  int lead;
  Buf(size_t bytes, int l) : lead(l) {
    const size_t all = (l + bytes + 15) / 16 * 16;
    raw = (char*)aligned_alloc(16, all ? all : 16);
    p = raw + l;
    memset(raw, 0xCD, l);
  }
  ~Buf() { free(raw); }
};

static int run(int G, int B, int max_blocks, int rep) {
  vector<int64_t> n(G), e(G), sno(G + 1, 0), seo(G + 1, 0);
  for (int g = 0; g < G; ++g) {
    n[g] = rng() % 4 ? rng() % 40 + 1 : rng() % 3;              // also graphs without nodes
    e[g] = n[g] ? (rng() % 4 ? rng() % 150 : rng() % 3) : 0;    // and without edges
    if (g == 0) { n[g] = 1; e[g] = 0; }
    sno[g + 1] = sno[g] + n[g];
    seo[g + 1] = seo[g] + e[g];
  }
  vector<int64_t> sel(B + 1, 0), dno(B + 1, 0), deo(B + 1, 0);
  for (int b = 0; b < B; ++b) {
    sel[b] = rep % 3 ? rng() % G : b % G;                       // every third run: in order (adjacent sources)
    dno[b + 1] = dno[b] + n[sel[b]];
    deo[b + 1] = deo[b] + e[sel[b]];
  }
  const int64_t N = dno[B], E = deo[B];
  const int NI = 10;
  const int rbs[NI] = {68, 36, 8, 128, 12, 164, 4, 8, 8, 8};
  const int kinds[NI] = {0, 0, 0, 1, 1, 1, 0, 2, 2, 3};
  vector<Buf*> src, dst;
  vector<vector<char>> want(NI);
  cgvp_collate_item items[NI];
  for (int i = 0; i < NI; ++i) {
    const bool node = kinds[i] == 0 || kinds[i] == 3;
    const int rb = rbs[i], unit = kinds[i] >= 2 ? 8 : 4;
    const int64_t srows = node ? sno[G] : seo[G], drows = node ? N : E;
    Buf* s = new Buf(srows * rb, (int)(rng() % (16 / unit)) * unit);
    Buf* d = new Buf(drows * rb, (int)(rng() % (16 / unit)) * unit);
    for (int64_t k = 0; k < srows * rb; ++k) s->p[k] = (char)rng();
    if (kinds[i] == 2)                                          // local node ids: small, so that + offset does not wrap
      for (int64_t r = 0; r < srows; ++r) {
        const int64_t v = (int64_t)(rng() % 1000);
        memcpy(s->p + 8 * r, &v, 8);
      }
    memset(d->p, 0xEE, drows * rb);
    want[i].resize(drows * rb);
    for (int b = 0; b < B; ++b) {
      const int64_t g = sel[b], cnt = node ? n[g] : e[g], so = node ? sno[g] : seo[g], d0 = node ? dno[b] : deo[b];
      for (int64_t r = 0; r < cnt; ++r) {
        if (kinds[i] < 2) {
          memcpy(&want[i][(d0 + r) * rb], s->p + (so + r) * rb, rb);
        } else {
          int64_t v = b;
          if (kinds[i] == 2) {
            uint64_t u;
            memcpy(&u, s->p + (so + r) * 8, 8);
            u += (uint64_t)dno[b];
            v = (int64_t)u;
          }
          memcpy(&want[i][(d0 + r) * 8], &v, 8);
        }
      }
    }
    items[i] = {d->p, kinds[i] == 3 ? nullptr : s->p, rb, kinds[i]};
    src.push_back(s);
    dst.push_back(d);
  }
  int bad = cgvp_collate_graphs(items, NI, sel.data(), dno.data(), deo.data(), sno.data(), seo.data(), B, N, E,
                                max_blocks, nullptr) != 0;
  for (int i = 0; i < NI; ++i) {
    if (!want[i].empty() && memcmp(dst[i]->p, want[i].data(), want[i].size())) {
      printf("item %d (row %d B, kind %d) differs: G %d B %d max_blocks %d\n", i, rbs[i], kinds[i], G, B, max_blocks);
      bad = 1;
    }
    for (int k = 0; k < dst[i]->lead; ++k)
      if ((unsigned char)dst[i]->raw[k] != 0xCD) { printf("item %d wrote in front of its destination\n", i); bad = 1; break; }
    delete src[i];
    delete dst[i];
  }
  return bad;
}

int main() {
  int bad = 0, rep = 0;
  for (int G : {1, 2, 5, 14})
    for (int B : {0, 1, 2, 3, 7, 64, 300})
      for (int max_blocks : {0, 1, 3})
        for (int k = 0; k < 3; ++k) bad |= run(G, B, max_blocks, rep++);
  printf(bad ? "FAILED\n" : "collate equals memcpy in %d runs\n", rep);
  return bad;
}
