// Native FLAC (RFC 9639; include/ttasr.h has the accepted stream): ONE decode body for the host and the device, and the host's
// container parser and frame scan.  decode_frame() is what ttasr_flac_decode runs frame after frame on the host and what
// flac_decode_kernel (kernels_ingest.hip) runs with one lane per FLAC frame; tests/flac_host_driver.cpp runs it under the
// address and undefined-behaviour sanitizers on damaged input.  Rules of the body: the bit reader never reads outside
// [frame begin, frame end) - past the end it yields zeros and remembers that -, every loop is bounded by a count or by the frame's
// end, every store by the blocksize the caller gave, and all sample arithmetic wraps (unsigned) so that a malformed stream has no
// undefined behaviour.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FLAC_HD __host__ __device__ inline
#else
#define FLAC_HD inline
#endif

namespace flac {

// what decode_frame returns: the per-frame status word
enum : int32_t {
  kOk = 0,
  kReserved = 1,        // reserved subframe type or residual method, a padding bit that is set; wasted bits that leave no sample width
  kBadLpc = 2,          // LPC precision 1111 or a negative shift
  kBadPartition = 3,    // a partition order that does not divide the blocksize, a partition or a block shorter than the order
  kPastEnd = 4,         // the subframes ran past the end of the frame (a unary run to the end, a cut frame)
  kHeader = 5,          // the frame header is invalid or disagrees with the table entry / the stream
  kLength = 6,          // the subframes end before the frame does
};

// why parse_header refuses
enum : int32_t {
  kHdrOk = 0, kHdrShort, kHdrSync, kHdrReservedBit, kHdrBlocksize, kHdrRate, kHdrChannels, kHdrBits, kHdrNumber, kHdrCrc8,
};

struct Stream { int32_t rate, channels, bits; };

struct Header {
  uint32_t blocksize;    // 1 ... 65535
  int32_t rate;          // 0: STREAMINFO's
  int32_t channels;      // 1 ... 8
  int32_t assignment;    // 0 independent, 8 left/side, 9 side/right, 10 mid/side
  int32_t bits;          // 0: STREAMINFO's
  int32_t variable;      // blocking strategy
  uint64_t number;       // frame number (fixed) or first-sample number (variable)
  uint32_t len;          // bytes of the header, CRC-8 included
};

FLAC_HD uint8_t crc8(const uint8_t* p, uint32_t n) {   // polynomial 0x07, init 0
  uint32_t c = 0;
  for (uint32_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
  }
  return (uint8_t)c;
}

// The frame header at p[0 .. n): fields, coded number and CRC-8.  Reads no byte from p + n on.  The codes that decide the header's
// length (blocksize and rate codes, the coded number's lead byte) are read first, then the CRC-8, then the reserved codes.
FLAC_HD int parse_header(const uint8_t* p, uint64_t n, Header& h) {
  if ((n >= 1 && p[0] != 0xFF) || (n >= 2 && (p[1] & 0xFE) != 0xF8)) return kHdrSync;
  if (n < 6) return kHdrShort;                       // sync and codes (4), the shortest number (1), CRC-8 (1)
  h.variable = p[1] & 1;
  const int bsc = p[2] >> 4, rc = p[2] & 15, cc = p[3] >> 4, sc = (p[3] >> 1) & 7;
  const uint32_t b = p[4];
  uint32_t extra;
  uint64_t v;
  if (b < 0x80) { extra = 0; v = b; }
  else if (b < 0xC0) return kHdrNumber;
  else if (b < 0xE0) { extra = 1; v = b & 0x1F; }
  else if (b < 0xF0) { extra = 2; v = b & 0x0F; }
  else if (b < 0xF8) { extra = 3; v = b & 0x07; }
  else if (b < 0xFC) { extra = 4; v = b & 0x03; }
  else if (b < 0xFE) { extra = 5; v = b & 0x01; }
  else if (b == 0xFE) { extra = 6; v = 0; }
  else return kHdrNumber;
  const uint32_t nbs = bsc == 6 ? 1 : (bsc == 7 ? 2 : 0), nrate = rc == 12 ? 1 : (rc == 13 || rc == 14 ? 2 : 0);
  const uint32_t len = 5 + extra + nbs + nrate + 1;
  if (n < len) return kHdrShort;
  for (uint32_t k = 0; k < extra; ++k) {
    const uint32_t c = p[5 + k];
    if ((c & 0xC0) != 0x80) return kHdrNumber;
    v = (v << 6) | (c & 0x3F);
  }
  h.number = v;
  h.len = len;
  // the CRC-8 first: a header whose CRC-8 holds IS a header, whatever its codes say (the scan tells a refusal from a coincidence by it)
  if (crc8(p, len - 1) != p[len - 1]) return kHdrCrc8;
  if (p[3] & 1) return kHdrReservedBit;
  if (bsc == 0) return kHdrBlocksize;
  if (rc == 15) return kHdrRate;
  if (cc > 10) return kHdrChannels;
  if (sc == 3) return kHdrBits;
  uint32_t at = 5 + extra;
  uint32_t bs;
  if (bsc == 1) bs = 192;
  else if (bsc <= 5) bs = 576u << (bsc - 2);
  else if (bsc == 6) { bs = (uint32_t)p[at] + 1; at += 1; }
  else if (bsc == 7) { bs = ((uint32_t)p[at] << 8 | p[at + 1]) + 1; at += 2; }
  else bs = 256u << (bsc - 8);
  if (bs > 65535) return kHdrBlocksize;
  h.blocksize = bs;
  int32_t rate = 0;
  switch (rc) {
    case 1: rate = 88200; break;
    case 2: rate = 176400; break;
    case 3: rate = 192000; break;
    case 4: rate = 8000; break;
    case 5: rate = 16000; break;
    case 6: rate = 22050; break;
    case 7: rate = 24000; break;
    case 8: rate = 32000; break;
    case 9: rate = 44100; break;
    case 10: rate = 48000; break;
    case 11: rate = 96000; break;
    case 12: rate = (int32_t)p[at] * 1000; at += 1; break;
    case 13: rate = (int32_t)((uint32_t)p[at] << 8 | p[at + 1]); at += 2; break;
    case 14: rate = (int32_t)((uint32_t)p[at] << 8 | p[at + 1]) * 10; at += 2; break;
    default: break;
  }
  if (rc != 0 && rate == 0) return kHdrRate;           // a coded rate of 0 Hz
  h.rate = rate;
  h.channels = cc < 8 ? cc + 1 : 2;
  h.assignment = cc < 8 ? 0 : cc;
  h.bits = sc == 0 ? 0 : (sc == 1 ? 8 : (sc == 2 ? 12 : (sc == 4 ? 16 : (sc == 5 ? 20 : (sc == 6 ? 24 : 32)))));
  return kHdrOk;
}

// MSB-first bit reader over p[0 .. n).  `cnt` low bits of `acc` are unread; bytes from n on read as zero.
struct Bits {
  const uint8_t* p;
  uint64_t n, bytepos, acc;
  int32_t cnt;

  FLAC_HD void refill() {                               // afterwards cnt is in [33, 64]
    if (cnt > 32) return;
    if (bytepos + 4 <= n) {                               // four bytes in one load while the frame has them
      uint32_t w;
      __builtin_memcpy(&w, p + bytepos, 4);
      acc = (acc << 32) | __builtin_bswap32(w);
      cnt += 32;
      bytepos += 4;
      return;
    }
    while (cnt <= 32) {
      const uint64_t b = bytepos < n ? p[bytepos] : 0;
      ++bytepos;
      acc = (acc << 8) | b;
      cnt += 8;
    }
  }
  FLAC_HD uint64_t consumed_bits() const { return bytepos * 8 - (uint64_t)cnt; }
  FLAC_HD bool over() const { return consumed_bits() > n * 8; }
  FLAC_HD uint32_t get(uint32_t k) {                    // k in [0, 32]
    if (k == 0) return 0;
    refill();
    cnt -= (int32_t)k;
    return (uint32_t)((acc >> cnt) & ((1ull << k) - 1));
  }
  FLAC_HD int32_t sget(uint32_t k) {                    // two's complement of k bits, k in [0, 32]
    if (k == 0) return 0;
    const uint32_t v = get(k);
    const uint32_t m = 1u << (k - 1);
    return (int32_t)((v ^ m) - m);
  }
  // zeros up to a one; false: the frame ended first
  FLAC_HD bool unary(uint32_t& q) {
    q = 0;
    for (;;) {
      refill();
      const uint64_t top = acc << (64 - cnt);           // cnt in [33, 64]: the unread bits from bit 63 down
      if (top) {
        const int32_t z = __builtin_clzll(top);
        q += (uint32_t)z;
        cnt -= z + 1;
        return !over();
      }
      q += (uint32_t)cnt;
      cnt = 0;
      if (bytepos >= n) return false;
    }
  }
  FLAC_HD uint32_t padding() { return get((uint32_t)cnt & 7); }   // the bits up to the next byte boundary (of bytepos * 8 - cnt)
};

FLAC_HD int32_t wrap_add(int32_t residual, int64_t pred) { return (int32_t)(uint32_t)((uint64_t)(int64_t)residual + (uint64_t)pred); }

// The predictor recurrence, s[i] = residual + ((sum_j coef[j] s[i - 1 - j]) >> shift), with its history where the compiler can keep
// it in registers: h[j] = s[i - 1 - j].  Every loop has the constant bound MAX (4: the fixed predictors, which are LPC with the
// coefficients below and shift 0; 12; 32) and a predicate on the order, so that no index is a run-time value.  The sum is int64:
// at most 32 products of 15 x 32 bits.
template <int MAX>
struct Pred {
  int32_t order, shift;
  int32_t coef[MAX], h[MAX];
  FLAC_HD int32_t next(int32_t e) {
    int64_t sum = 0;
#pragma unroll
    for (int j = 0; j < MAX; ++j)
      if (j < order) sum += (int64_t)coef[j] * (int64_t)h[j];
    const int32_t v = wrap_add(e, sum >> shift);
#pragma unroll
    for (int j = MAX - 1; j > 0; --j)
      if (j < order) h[j] = h[j - 1];
    h[0] = v;
    return v;
  }
};

// The residual of a predicted subframe, each value through the predictor as it is decoded: s[order .. bs) = samples << wasted.
template <int MAX>
FLAC_HD int residual(Bits& br, int32_t* s, uint32_t bs, uint32_t order, Pred<MAX>& pd, uint32_t wasted) {
  const uint32_t method = br.get(2);
  if (method > 1) return kReserved;
  const uint32_t P = br.get(4), parts = 1u << P, per = bs >> P;
  if ((bs & (parts - 1)) || per < order) return kBadPartition;
  const uint32_t pb = method ? 5 : 4, esc = (1u << pb) - 1;
  uint32_t i = order;
  for (uint32_t part = 0; part < parts; ++part) {
    const uint32_t count = per - (part == 0 ? order : 0);
    const uint32_t k = br.get(pb);
    if (k == esc) {
      const uint32_t nb = br.get(5);
      for (uint32_t j = 0; j < count; ++j) s[i++] = (int32_t)((uint32_t)pd.next(br.sget(nb)) << wasted);
    } else {
      for (uint32_t j = 0; j < count; ++j) {
        uint32_t q;
        if (!br.unary(q)) return kPastEnd;
        const uint32_t u = (q << k) | br.get(k);
        s[i++] = (int32_t)((uint32_t)pd.next((int32_t)((u >> 1) ^ (0u - (u & 1)))) << wasted);
      }
    }
    if (br.over()) return kPastEnd;
  }
  return kOk;
}

// Warm-up samples, LPC parameters (lpc) or the fixed predictor's coefficients, then the residual.
template <int MAX>
FLAC_HD int predicted(Bits& br, int32_t* s, uint32_t bs, uint32_t order, uint32_t w, uint32_t wasted, bool lpc) {
  Pred<MAX> pd;
  pd.order = (int32_t)order;
  pd.shift = 0;
#pragma unroll
  for (int j = 0; j < MAX; ++j) { pd.coef[j] = 0; pd.h[j] = 0; }
  for (uint32_t i = 0; i < order; ++i) {
    const int32_t v = br.sget(w);
    s[i] = (int32_t)((uint32_t)v << wasted);
#pragma unroll
    for (int j = MAX - 1; j > 0; --j) pd.h[j] = pd.h[j - 1];       // newest first
    pd.h[0] = v;
  }
  if (lpc) {
    const uint32_t prec = br.get(4) + 1;
    if (prec == 16) return kBadLpc;
    pd.shift = br.sget(5);
    if (pd.shift < 0) return kBadLpc;
    for (uint32_t i = 0; i < order; ++i) {
      const int32_t cf = br.sget(prec);
#pragma unroll
      for (int j = 0; j < MAX; ++j)
        if ((uint32_t)j == i) pd.coef[j] = cf;
    }
  } else {
    const int32_t fixed[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
#pragma unroll
    for (int j = 0; j < 4 && j < MAX; ++j) pd.coef[j] = fixed[order][j];
  }
  return residual<MAX>(br, s, bs, order, pd, wasted);
}

// One subframe of `bps` bits per sample -> s[0 .. bs), the wasted-bits shift applied.
FLAC_HD int subframe(Bits& br, int32_t* s, uint32_t bs, uint32_t bps) {
  if (br.get(1)) return kReserved;
  const uint32_t type = br.get(6);
  uint32_t wasted = 0;
  if (br.get(1)) {
    if (!br.unary(wasted)) return kPastEnd;
    ++wasted;
  }
  if (wasted >= bps) return kReserved;
  const uint32_t w = bps - wasted;
  int e = kOk;
  if (type == 0) {
    const int32_t v = (int32_t)((uint32_t)br.sget(w) << wasted);
    for (uint32_t i = 0; i < bs; ++i) s[i] = v;
  } else if (type == 1) {
    for (uint32_t i = 0; i < bs; ++i) {
      s[i] = (int32_t)((uint32_t)br.sget(w) << wasted);
      if ((i & 255) == 255 && br.over()) return kPastEnd;
    }
  } else if (type >= 8 && type <= 12) {
    if (type - 8 > bs) return kBadPartition;
    e = predicted<4>(br, s, bs, type - 8, w, wasted, false);
  } else if (type >= 32) {
    const uint32_t order = type - 31;
    if (order > bs) return kBadPartition;
    e = order <= 4 ? predicted<4>(br, s, bs, order, w, wasted, true)
                   : (order <= 12 ? predicted<12>(br, s, bs, order, w, wasted, true) : predicted<32>(br, s, bs, order, w, wasted, true));
  } else {
    return kReserved;
  }
  if (e) return e;
  return br.over() ? kPastEnd : kOk;
}

enum : int32_t { kStorePlain = 0, kStoreS16 = 1, kStoreS32 = 2 };   // int32 values | left-justified int16 | left-justified int32

// One FLAC frame p[0 .. n) (sync to CRC-16) of a stream `si` whose table entry says `want_bs` samples: the subframes into
// work[channels][want_bs], then decorrelation and the store of out[want_bs][channels] in `store`.  Returns the status word.
FLAC_HD int decode_frame(const uint8_t* __restrict__ p, uint64_t n, const Stream& si, uint32_t want_bs, int32_t* __restrict__ work,
                         void* __restrict__ out, int32_t store) {
  Header h;
  if (parse_header(p, n, h) != kHdrOk) return kHeader;
  if (h.blocksize != want_bs || (h.rate && h.rate != si.rate) || h.channels != si.channels || (h.bits && h.bits != si.bits) ||
      si.bits < 4 || si.bits > 24 || si.channels < 1 || si.channels > 8)
    return kHeader;
  const uint32_t bs = want_bs, ch = (uint32_t)si.channels;
  Bits br{p, n, h.len, 0, 0};
  for (uint32_t c = 0; c < ch; ++c) {
    const bool side = (h.assignment == 8 && c == 1) || (h.assignment == 9 && c == 0) || (h.assignment == 10 && c == 1);
    const int e = subframe(br, work + (size_t)c * bs, bs, (uint32_t)si.bits + (side ? 1 : 0));
    if (e) return e;
  }
  if (br.padding()) return kReserved;
  const uint64_t used = br.consumed_bits() / 8 + 2;      // the CRC-16 follows the padding
  if (used != n) return used > n ? kPastEnd : kLength;
  const uint32_t sh16 = 16 - (uint32_t)(si.bits <= 16 ? si.bits : 16), sh32 = 32 - (uint32_t)si.bits;
  for (uint32_t i = 0; i < bs; ++i) {
    if (h.assignment) {
      const uint32_t a = (uint32_t)work[i], b = (uint32_t)work[bs + i];
      uint32_t l, r;
      if (h.assignment == 8) { l = a; r = a - b; }
      else if (h.assignment == 9) { l = a + b; r = b; }
      else {
        const uint32_t m = (a << 1) | (b & 1);
        l = (uint32_t)((int32_t)(m + b) >> 1);
        r = (uint32_t)((int32_t)(m - b) >> 1);
      }
      work[i] = (int32_t)l;
      work[bs + i] = (int32_t)r;
    }
    for (uint32_t c = 0; c < ch; ++c) {
      const uint32_t v = (uint32_t)work[(size_t)c * bs + i];
      const size_t at = (size_t)i * ch + c;
      if (store == kStoreS16) ((int16_t*)out)[at] = (int16_t)(uint16_t)(v << sh16);
      else if (store == kStoreS32) ((int32_t*)out)[at] = (int32_t)(v << sh32);
      else ((int32_t*)out)[at] = (int32_t)v;
    }
  }
  return kOk;
}

}  // namespace flac

// ---- host only: the container and the frame scan ----
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

namespace flac {

inline const char* status_text(int e) {
  switch (e) {
    case kOk: return "ok";
    case kReserved: return "reserved subframe type or field";
    case kBadLpc: return "bad LPC precision or shift";
    case kBadPartition: return "bad residual partition";
    case kPastEnd: return "the subframes run past the end of the frame";
    case kHeader: return "the frame header disagrees with the stream";
    case kLength: return "the subframes end before the frame does";
    default: return "unknown";
  }
}

inline const char* header_text(int e) {
  switch (e) {
    case kHdrShort: return "cut inside the frame header";
    case kHdrSync: return "no frame sync";
    case kHdrReservedBit: return "reserved bit set";
    case kHdrBlocksize: return "reserved blocksize code";
    case kHdrRate: return "invalid rate code";
    case kHdrChannels: return "reserved channel code";
    case kHdrBits: return "reserved sample-size code";
    case kHdrNumber: return "invalid coded number";
    case kHdrCrc8: return "broken header CRC-8";
    default: return "ok";
  }
}

struct FrameRec { int64_t off, len, first; uint32_t bs; };

struct Probe {
  Stream si{0, 0, 0};
  int64_t total_claim = 0, first_frame = 0, end = 0, samples = 0;
  uint32_t max_bs = 0;
  bool md5 = false;
  std::vector<FrameRec> frames;
};

// CRC-16, polynomial 0x8005, MSB first, eight bytes per step: t[k][b] is the CRC of byte b followed by k zero bytes
struct Crc16 {
  uint16_t t[8][256];
  Crc16() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i << 8;
      for (int k = 0; k < 8; ++k) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
      t[0][i] = (uint16_t)c;
    }
    for (int k = 1; k < 8; ++k)
      for (uint32_t i = 0; i < 256; ++i) t[k][i] = (uint16_t)(((uint32_t)t[k - 1][i] << 8) ^ t[0][t[k - 1][i] >> 8]);
  }
  uint32_t run(uint32_t crc, const uint8_t* p, int64_t n) const {
    for (; n >= 8; p += 8, n -= 8)
      crc = t[7][p[0] ^ (crc >> 8)] ^ t[6][p[1] ^ (crc & 0xFF)] ^ t[5][p[2]] ^ t[4][p[3]] ^ t[3][p[4]] ^ t[2][p[5]] ^ t[1][p[6]] ^ t[0][p[7]];
    for (; n > 0; ++p, --n) crc = ((crc << 8) ^ t[0][((crc >> 8) ^ *p) & 0xFF]) & 0xFFFF;
    return crc;
  }
};
inline const Crc16& crc16() { static const Crc16 c; return c; }

// nullptr: the header fits the stream; otherwise what differs
inline const char* stream_mismatch(const Header& h, const Stream& si) {
  if (h.rate && h.rate != si.rate) return "its rate differs from STREAMINFO's";
  if (h.channels != si.channels) return "its channel count differs from STREAMINFO's";
  if (h.bits == 32) return "32 bits per sample (25 to 32 are not supported)";
  if (h.bits && h.bits != si.bits) return "its sample width differs from STREAMINFO's";
  return nullptr;
}

inline bool continues(const Header& prev, const Header& h) {
  if (h.variable != prev.variable) return false;
  return h.number == (prev.variable ? prev.number + prev.blocksize : prev.number + 1);
}

// printf into the optional message buffer
__attribute__((format(printf, 3, 4))) inline void say(char* why, int32_t len, const char* fmt, ...) {
  if (!why || len <= 0) return;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(why, (size_t)len, fmt, ap);
  va_end(ap);
}

constexpr int64_t kMaxSamples = (int64_t)1 << 40;

// The whole file as read -> STREAMINFO and the frame table.  false: refused, `why` says which rule.  `max_samples` is the most
// samples per channel a file may hold (the tests lower it).
inline bool scan(const uint8_t* p, int64_t n, Probe& P, char* why, int32_t len, int64_t max_samples = kMaxSamples) {
  if (why && len > 0) why[0] = 0;
  int64_t pos = 0;
  if (n >= 10 && !memcmp(p, "ID3", 3)) {
    const int64_t size = (int64_t)(p[6] & 0x7F) << 21 | (int64_t)(p[7] & 0x7F) << 14 | (int64_t)(p[8] & 0x7F) << 7 | (p[9] & 0x7F);
    pos = 10 + size + ((p[5] & 0x10) ? 10 : 0);
  }
  if (pos + 4 > n || memcmp(p + pos, "fLaC", 4)) { say(why, len, "no fLaC marker at byte %lld", (long long)pos); return false; }
  pos += 4;
  bool last = false, first = true;
  while (!last) {
    if (pos + 4 > n) { say(why, len, "cut inside the metadata at byte %lld", (long long)pos); return false; }
    const int type = p[pos] & 0x7F;
    last = (p[pos] & 0x80) != 0;
    const int64_t size = (int64_t)p[pos + 1] << 16 | (int64_t)p[pos + 2] << 8 | p[pos + 3];
    if (type == 127) { say(why, len, "metadata block type 127 at byte %lld is invalid", (long long)pos); return false; }
    if (first != (type == 0)) { say(why, len, "STREAMINFO must be the first metadata block and the only one of its type (byte %lld)", (long long)pos); return false; }
    pos += 4;
    if (pos + size > n) { say(why, len, "cut inside the metadata block at byte %lld", (long long)(pos - 4)); return false; }
    if (first) {
      if (size != 34) { say(why, len, "STREAMINFO of %lld bytes instead of 34", (long long)size); return false; }
      const uint8_t* s = p + pos;
      P.si.rate = (int32_t)((uint32_t)s[10] << 12 | (uint32_t)s[11] << 4 | s[12] >> 4);
      P.si.channels = ((s[12] >> 1) & 7) + 1;
      P.si.bits = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
      P.total_claim = (int64_t)(s[13] & 15) << 32 | (int64_t)s[14] << 24 | (int64_t)s[15] << 16 | (int64_t)s[16] << 8 | s[17];
      P.md5 = false;
      for (int k = 0; k < 16; ++k) P.md5 = P.md5 || s[18 + k] != 0;
      if (P.si.bits > 24) { say(why, len, "%d bits per sample (25 to 32 are not supported)", P.si.bits); return false; }
      if (P.si.bits < 4) { say(why, len, "%d bits per sample (below 4)", P.si.bits); return false; }
      if (P.si.rate == 0) { say(why, len, "STREAMINFO with rate 0"); return false; }
      first = false;
    }
    pos += size;
  }
  P.first_frame = pos;
  int64_t end = n;
  if (end - 128 >= pos && !memcmp(p + end - 128, "TAG", 3)) end -= 128;
  P.end = end;
  P.frames.clear();
  P.samples = 0;
  P.max_bs = 0;
  const Crc16& K = crc16();
  Header h;
  if (pos < end) {
    const int r = parse_header(p + pos, (uint64_t)(end - pos), h);
    if (r) { say(why, len, "frame 0 at byte %lld: %s", (long long)pos, header_text(r)); return false; }
    if (const char* m = stream_mismatch(h, P.si)) { say(why, len, "frame 0 at byte %lld: %s", (long long)pos, m); return false; }
  }
  // A place where the CRC-16 holds and a sync code stands, but no valid continuing header: by the definition not a frame end, and
  // passed over.  It is kept for the refusal's message - when the stream is damaged there, it is where the next frame should begin.
  struct Suspect { int64_t at; char msg[160]; };
  constexpr size_t kSuspects = 8;
  std::vector<Suspect> sus;
  std::vector<int32_t> trial;                               // work rows and output of a trial decode
  auto decodes = [&](int64_t from, int64_t to, uint32_t bs) {
    const size_t vals = (size_t)bs * (size_t)P.si.channels;
    trial.resize(2 * vals);
    return decode_frame(p + from, (uint64_t)(to - from), P.si, bs, trial.data(), trial.data() + vals, kStorePlain) == kOk;
  };
  while (pos < end) {
    // `h` is the valid header at pos; the frame ends at the smallest q whose CRC-16 holds and where the data end or a valid
    // continuing header begins.  Only a q where a sync code begins, or the end of the data, can be such a q: the CRC runs in bulk
    // from one to the next.
    uint32_t crc = 0;
    int64_t done = pos, q = pos + (int64_t)h.len + 3, found = -1, junk = -1;
    Header g{};
    const long long k = (long long)P.frames.size();
    sus.clear();
    while (found < 0) {
      int64_t cand = end;
      for (int64_t f = q; f < end - 1;) {
        const uint8_t* hit = (const uint8_t*)memchr(p + f, 0xFF, (size_t)(end - 1 - f));
        if (!hit) break;
        if ((hit[1] & 0xFE) == 0xF8) { cand = hit - p; break; }
        f = hit - p + 1;
      }
      if (cand < done) break;                               // (a frame too short to hold a subframe and its CRC, at the end)
      crc = K.run(crc, p + done, cand - done);
      done = cand;
      q = cand + 1;
      if (cand == end) { if (crc == 0 && cand - pos >= (int64_t)h.len + 3) found = cand; break; }
      if (crc != 0 || cand - pos < (int64_t)h.len + 3) continue;
      const int r = parse_header(p + cand, (uint64_t)(end - cand), g);
      const char* m = r ? header_text(r) : stream_mismatch(g, P.si);
      if (!m && continues(h, g)) { found = cand; break; }
      if (sus.size() == kSuspects) continue;
      Suspect u;
      u.at = cand;
      if (m) snprintf(u.msg, sizeof u.msg, "frame %lld at byte %lld: %s", k + 1, (long long)cand, m);
      else snprintf(u.msg, sizeof u.msg, "frame %lld at byte %lld: its coded number %llu does not continue %llu (%s blocking, %u samples before it)", k + 1,
                    (long long)cand, (unsigned long long)g.number, (unsigned long long)h.number, h.variable ? "variable" : "fixed", h.blocksize);
      sus.push_back(u);
    }
    // Suspects were passed over: when the frame so found does not decode and the bytes up to a suspect do, frames were swallowed
    // behind a damaged header, and the suspect is what is wrong with the file.  Without a suspect that explains it the frame
    // stands as the definition finds it, and its content is the decoder's to judge.
    if (!sus.empty() && !(found >= 0 && decodes(pos, found, h.blocksize))) {
      const Suspect* blame = found < 0 ? &sus[0] : nullptr;
      for (const Suspect& u : sus)
        if (decodes(pos, u.at, h.blocksize)) { blame = &u; break; }
      if (blame) { say(why, len, "%s", blame->msg); return false; }
    }
    if (found < 0) {   // for the message: is there a place where the CRC-16 holds and no frame follows?
      uint32_t c2 = 0;
      for (int64_t j = pos; j < end - 1 && junk < 0; ++j) {
        c2 = K.run(c2, p + j, 1);
        if (c2 == 0 && j + 1 - pos >= (int64_t)h.len + 3) junk = j + 1;
      }
      if (junk >= 0) say(why, len, "%lld bytes behind frame %lld (from byte %lld) are neither a frame nor an ID3v1 tag", (long long)(end - junk), k, (long long)junk);
      else say(why, len, "frame %lld at byte %lld: no end where its CRC-16 holds (a broken CRC or a cut file)", k, (long long)pos);
      return false;
    }
    if (P.samples + h.blocksize > max_samples) {
      if (max_samples == kMaxSamples) say(why, len, "more than 2^40 samples");
      else say(why, len, "more than %lld samples", (long long)max_samples);
      return false;
    }
    P.frames.push_back(FrameRec{pos, found - pos, P.samples, h.blocksize});
    P.samples += h.blocksize;
    if (h.blocksize > P.max_bs) P.max_bs = h.blocksize;
    pos = found;
    h = g;
  }
  return true;
}

}  // namespace flac
