// share_order.hpp — where the units of one trip-count class go in the "share order" (stag_plan_share*), for the host
// builder and the device builder alike: plain integer code, no HIP in it.
//
// A class occupies the absolute unit indices [a, b) of the plan.  Its units arrive RANKED: the members of complete
// octets first (8 ranks each, the two quads of an octet and the two pairs of a quad side by side), then of the quads,
// the pairs, the single units.  share_layout decides, from the cluster counts, which clusters fill the hole in front of
// the first multiple of 8 — single units, then pairs, then a quad, so that each starts on a multiple of its size — and
// share_position maps a rank to its index.  Where the hole needs a smaller cluster than there is, the LAST cluster of
// the next larger size is taken apart (its halves are the first ranks of the smaller size).  A class that ends inside the
// block of 8 it starts in keeps its pairs (a quad counts as two), on even indices, and no larger group.
#ifndef STAG_SHARE_ORDER_HPP
#define STAG_SHARE_ORDER_HPP

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STAG_SHARE_HD __host__ __device__
#else
#define STAG_SHARE_HD
#endif

// sort key of a whole-row unit inside the builders: class index (lengths descending) | size code (0: octet ... 3: single)
// | cluster id (its smallest member's unit index) | member offset inside the cluster
constexpr int kShareOffBits = 3, kShareIdBits = 31, kShareSizeBits = 2, kShareClassBits = 20;
constexpr int kShareSizeShift = kShareOffBits + kShareIdBits;            // 34
constexpr int kShareClassShift = kShareSizeShift + kShareSizeBits;       // 36
constexpr int kShareKeyBits = kShareClassShift + kShareClassBits;        // 56
constexpr int kShareLevels = 3;                                          // 1 -> 2 -> 4 -> 8

STAG_SHARE_HD inline int32_t share_trips(int32_t len) { return (len + 1) / 2; }

// class index of a whole-row unit: 0 for the longest rows a plan of this seg_len can have
STAG_SHARE_HD inline int32_t share_class(int32_t len, int32_t seg_len) {
  const int32_t c = share_trips(seg_len) - share_trips(len < 0 ? 0 : len);
  return c < 0 ? 0 : c;
}

STAG_SHARE_HD inline uint64_t share_unit_key(int32_t cls, int32_t level, int32_t cid, int32_t off) {
  return ((uint64_t)(uint32_t)cls << kShareClassShift) | ((uint64_t)(uint32_t)(kShareLevels - level) << kShareSizeShift) |
         ((uint64_t)(uint32_t)cid << kShareOffBits) | (uint64_t)(uint32_t)off;
}

// the same hash on both builders' candidate pairs (the device builder takes the smallest per cluster)
STAG_SHARE_HD inline uint32_t share_hash(uint32_t a, uint32_t b, uint32_t salt) {
  uint32_t h = a * 0x9E3779B1u ^ b * 0x85EBCA77u ^ salt * 0xC2B2AE3Du;
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

struct ShareLayout {
  int32_t a;        // first index of the class
  int32_t body;     // first index behind the hole: where the clusters go in descending size
  int32_t cnt[4];   // clusters of 8, 4, 2, 1 units after taking apart
  int32_t w[4];     // how many of them fill the hole
};

STAG_SHARE_HD inline ShareLayout share_layout(int32_t a, int32_t b, int32_t c8, int32_t c4, int32_t c2, int32_t c1) {
  ShareLayout L;
  L.a = a;
  L.cnt[0] = c8; L.cnt[1] = c4; L.cnt[2] = c2; L.cnt[3] = c1;
  L.w[0] = L.w[1] = L.w[2] = L.w[3] = 0;
  const int32_t a8 = (a + 7) & ~7;
  if (a8 > a && a8 >= b) {
    // fewer than 8 units, inside one block: pairs and single units only, around the most aligned index of [a, b]
    int32_t p = a;
    for (int32_t q = a + 1; q <= b; ++q)
      if ((q & -q) > (p & -p)) p = q;
    const int32_t h = p - a, room = h / 2 + (b - p) / 2;
    L.cnt[2] += 2 * L.cnt[1];
    L.cnt[0] = L.cnt[1] = 0;
    if (L.cnt[2] > room) { L.cnt[3] += 2 * (L.cnt[2] - room); L.cnt[2] = room; }
    L.w[2] = L.cnt[2] < h / 2 ? L.cnt[2] : h / 2;
    L.w[3] = (h & 1) + 2 * (h / 2 - L.w[2]);
    L.body = p;
    return L;
  }
  const int32_t h = a8 - a;
  L.w[1] = (h >> 2) & 1; L.w[2] = (h >> 1) & 1; L.w[3] = h & 1;
  for (int t = 1; t < 4; ++t) {
    while (L.cnt[t] < L.w[t]) {
      int j = t - 1;
      while (j >= 0 && L.cnt[j] <= L.w[j]) --j;       // the nearest larger size with a cluster to spare
      if (j < 0) break;
      L.cnt[j] -= 1;
      L.cnt[j + 1] += 2;
    }
    if (L.cnt[t] < L.w[t]) {                          // none: twice as many of the next smaller size (b - a >= h: they exist)
      if (t < 3) L.w[t + 1] += 2 * (L.w[t] - L.cnt[t]);
      L.w[t] = L.cnt[t];
    }
  }
  L.body = a8;
  return L;
}

STAG_SHARE_HD inline int32_t share_position(const ShareLayout& L, int32_t r) {
  const int32_t hole[4] = {L.a, L.a + L.w[3] + 2 * L.w[2], L.a + L.w[3], L.a};
  int32_t first = 0, body = L.body;
  for (int t = 0; t < 4; ++t) {
    const int32_t sz = 8 >> t, n = L.cnt[t] * sz;
    if (r < first + n || t == 3) {
      const int32_t o = r - first, i = o / sz, m = o % sz;
      return (i < L.w[t] ? hole[t] + i * sz : body + (i - L.w[t]) * sz) + m;
    }
    first += n;
    body += (L.cnt[t] - L.w[t]) * sz;
  }
  return L.a + r;
}

#endif
