// libttasr: the three context-free FLAC entry points (include/ttasr.h ttasr_flac_probe / ttasr_flac_frames / ttasr_flac_decode).
// No GPU, no context: the container parser and frame scan of flac.hpp, and its decode body run frame after frame on the calling
// thread.  The device runs the same body (kernels_ingest.hip flac_decode_kernel).
#include <new>

#include "../../include/ttasr.h"
#include "flac.hpp"

namespace {

template <class F>
int64_t flac_guarded(char* why, int32_t len, F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    flac::say(why, len, "out of memory");
    return TTASR_E_NOMEM;
  } catch (...) {
    flac::say(why, len, "unexpected exception");
    return TTASR_E_INVALID;
  }
}

bool flac_args(const void* bytes, int64_t n_bytes, char* why, int32_t len) {
  if (why && len > 0) why[0] = 0;
  if (!bytes || n_bytes < 0) { flac::say(why, len, "NULL bytes or a negative length"); return false; }
  return true;
}

}  // namespace

extern "C" {

int ttasr_flac_probe(const void* bytes, int64_t n_bytes, int64_t* out, char* why, int32_t len) {
  return (int)flac_guarded(why, len, [&]() -> int64_t {
    if (!flac_args(bytes, n_bytes, why, len)) return TTASR_E_INVALID;
    if (!out) { flac::say(why, len, "NULL out"); return TTASR_E_INVALID; }
    flac::Probe P;
    if (!flac::scan((const uint8_t*)bytes, n_bytes, P, why, len)) return TTASR_E_INVALID;
    out[0] = P.si.rate; out[1] = P.si.channels; out[2] = P.si.bits; out[3] = P.samples;
    out[4] = (int64_t)P.frames.size(); out[5] = P.max_bs; out[6] = P.first_frame;
    out[7] = (P.md5 ? 1 : 0) | (P.total_claim != 0 && P.total_claim != P.samples ? 2 : 0);
    return TTASR_OK;
  });
}

int64_t ttasr_flac_frames(const void* bytes, int64_t n_bytes, int64_t* table, int64_t cap, char* why, int32_t len) {
  return flac_guarded(why, len, [&]() -> int64_t {
    if (!flac_args(bytes, n_bytes, why, len)) return TTASR_E_INVALID;
    flac::Probe P;
    if (!flac::scan((const uint8_t*)bytes, n_bytes, P, why, len)) return TTASR_E_INVALID;
    const int64_t n = (int64_t)P.frames.size();
    for (int64_t k = 0; table && k < n && k < cap; ++k) {
      table[3 * k] = P.frames[k].off; table[3 * k + 1] = P.frames[k].len; table[3 * k + 2] = P.frames[k].first;
    }
    return n;
  });
}

int64_t ttasr_flac_decode(const void* bytes, int64_t n_bytes, int32_t* out, int64_t cap_samples, char* why, int32_t len) {
  return flac_guarded(why, len, [&]() -> int64_t {
    if (!flac_args(bytes, n_bytes, why, len)) return TTASR_E_INVALID;
    flac::Probe P;
    if (!flac::scan((const uint8_t*)bytes, n_bytes, P, why, len)) return TTASR_E_INVALID;
    if (P.samples > cap_samples || (P.samples > 0 && !out)) {
      flac::say(why, len, "%lld samples per channel are held, the output takes %lld", (long long)P.samples, (long long)cap_samples);
      return TTASR_E_INVALID;
    }
    std::vector<int32_t> work((size_t)P.max_bs * P.si.channels);
    for (size_t k = 0; k < P.frames.size(); ++k) {
      const flac::FrameRec& f = P.frames[k];
      const int e = flac::decode_frame((const uint8_t*)bytes + f.off, (uint64_t)f.len, P.si, f.bs, work.data(),
                                       out + (size_t)f.first * P.si.channels, flac::kStorePlain);
      if (e) { flac::say(why, len, "frame %zu at byte %lld: %s", k, (long long)f.off, flac::status_text(e)); return TTASR_E_INVALID; }
    }
    return P.samples;
  });
}

}  // extern "C"
