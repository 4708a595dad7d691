// What the stand-alone op entry points share (op_shims.hip, op_shims_conv.hip; odt_nn_cosine in tracker.hip takes set_dev):
// the one owner of their temporary device memory, the host <-> device copies, the range-slot helpers and the conv helpers
// that cross the two files.  Host code only.
#pragma once
#include "odt_model.hpp"

namespace odt {

inline int set_dev(int device) {
  int n = 0;
  ODT_HIP(hipGetDeviceCount(&n));
  ODT_CHECK(device >= 0 && device < n, "no such device");
  ODT_HIP(hipSetDevice(device));
  return 0;
}

// Device buffers of an odt_op_* call -- inputs, outputs, scratch, weight images, uploaded records: every one ends in
// kGuardBytes of sentinel bytes, and check() reports -- by the buffer's name -- a launch that wrote into them.  There is no
// sanitizer on the device: this turns a write past the end of an output or scratch buffer into an error of the call.
// A buffer nothing initialises starts as sentinel bytes too (an element no kernel wrote reads back as 0x7F7F7F7F, 3.39e38),
// except where the plan zero-initialises the buffer and relies on that (range slots, the squeeze-excite gate).
constexpr size_t kGuardBytes = 1024;
constexpr int kGuardByte = 0x7F;

struct GBufs {
  struct Buf { unsigned char* d = nullptr; size_t bytes = 0; std::string name; };
  std::vector<Buf> v;
  GBufs() = default;
  GBufs(const GBufs&) = delete;
  GBufs& operator=(const GBufs&) = delete;
  // the launches of a call may still be in flight on any way out of it (run_conv returns without waiting)
  ~GBufs() {
    (void)hipDeviceSynchronize();
    for (const Buf& b : v) if (b.d) (void)hipFree(b.d);
  }
  // count elements: a copy of `host`, or filled with `fill` (a byte value) or the sentinel (fill < 0); then the guard.
  // *out may be a pointer to const: a params field the kernels only read
  template <typename T>
  int alloc(const std::string& name, size_t count, T** out, int fill = -1, const void* host = nullptr) {
    v.emplace_back();
    Buf& g = v.back();
    g.name = name; g.bytes = count * sizeof(T);
    ODT_HIP(hipMalloc((void**)&g.d, g.bytes + kGuardBytes));
    if (host != nullptr) { ODT_HIP(hipMemcpy(g.d, host, g.bytes, hipMemcpyHostToDevice)); }
    else { ODT_HIP(hipMemset(g.d, fill < 0 ? kGuardByte : fill, g.bytes)); }
    ODT_HIP(hipMemset(g.d + g.bytes, kGuardByte, kGuardBytes));
    *out = reinterpret_cast<T*>(g.d);
    return 0;
  }
  // after the launches: synchronise, then every guard region must still hold the sentinel
  int check(const char* op) {
    ODT_HIP(hipDeviceSynchronize());
    std::vector<unsigned char> h(kGuardBytes);
    for (const Buf& g : v) {
      ODT_HIP(hipMemcpy(h.data(), g.d + g.bytes, kGuardBytes, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < kGuardBytes; ++i)
        ODT_CHECK(h[i] == (unsigned char)kGuardByte, std::string(op) + ": write past the end of " + g.name + " (guard byte " +
                                                         std::to_string(i) + ")");
    }
    return 0;
  }
};

template <typename T>
int get_dev(T* host, const T* dev, size_t count) {
  if (host != nullptr && count > 0) ODT_HIP(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost));
  return 0;
}

// `slots` range slots in a row (kAmaxWays words each, which the kernels max-reduce into), zeroed as a plan zeroes its own
inline int alloc_amax(GBufs& g, unsigned** slot, int slots = 1) {
  return g.alloc("range slot", (size_t)slots * kAmaxWays, slot, 0);
}
// ... and the |max| one slot recorded
inline int read_amax(const unsigned* slot, float* amax) {
  unsigned bits[kAmaxWays], a = 0u;
  ODT_HIP(hipMemcpy(bits, slot, sizeof(bits), hipMemcpyDeviceToHost));
  for (unsigned b : bits) a = b > a ? b : a;
  std::memcpy(amax, &a, 4);
  return 0;
}

// op_shims_conv.hip
void note_conv(const ConvParams& q);      // odt_op_last_conv reports this record's row and launch choices
ConvParams same_conv(const float* in, const float* wt, const float* bias, float* out, int B, int H, int W, int Cin, int Cout, int k,
                     int dil, int relu);
std::vector<float> ohwi(const float* hwio, int kh, int kw, int Cin, int Cout);
int run_conv(GBufs& g, ConvParams q, const Knobs& kn);

}  // namespace odt
