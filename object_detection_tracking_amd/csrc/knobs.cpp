// The one reader of the ODT_* environment overrides (knobs.hpp).
#include "knobs.hpp"

#include <cstdlib>

namespace odt {
namespace {

const char* const kNames[K_COUNT] = {
#define ODT_KNOB_NAME(n) "ODT_" #n,
    ODT_KNOB_LIST(ODT_KNOB_NAME)
#undef ODT_KNOB_NAME
};

}  // namespace

Knobs knobs_read() {
  Knobs t;
  for (int k = 0; k < K_COUNT; ++k) {
    const char* e = getenv(kNames[k]);
    if (e != nullptr) { t.v[k].set = true; t.v[k].i = atol(e); t.v[k].d = atof(e); t.v[k].c0 = e[0]; t.text[k] = e; }
  }
  return t;
}

std::vector<std::string> Knobs::active() const {
  std::vector<std::string> out;
  for (int k = 0; k < K_COUNT; ++k)
    if (v[k].set) out.push_back(std::string(kNames[k]) + "=" + text[k]);
  return out;
}

}  // namespace odt
