// Test-only harness around the two kernels of csrc/random_voice.h (included unchanged, kernels and launch helpers only): rlg_layer_kernel, one layer of
// upstream's RandomLatentConverter, and rlg_noise_kernel, its input noise. Host arrays in, host arrays out, ONE launch per call on a stream of its own, through
// rlg_launch_layer / rlg_launch_noise, the very functions the product launches with, so that the grid, the block and the LDS size are the product's. Built as
// libtts_rlg_test.so next to the product library; not part of the product (tests/test_rlg_kernels_gpu.py and tests/test_rlg_harness_cpu.py are the only users).
//
// THE MEMORY CONTRACT. The kernels check no bounds; they rely on what random_voice.h's callers guarantee:
//   dim      a multiple of 256 from RLG_MIN_DIM (256, the smallest the kernel accepts: a row is read as 64 lanes x float4) to RLG_MAX_DIM (2048: the batch
//            tile's activations fill 64 KB of LDS); w [dim][dim], bias [dim], x and y [n][dim], all 16-byte aligned.
//   n        >= 1; rows of x at or beyond n are never read, rows of y at or beyond n never written (the last batch tile may be partial).
// The GPU is shared: a case is validated completely BEFORE any HIP call and everything else is refused; every device buffer is margin | payload | margin in one
// allocation; x is allocated with whole batch tiles, the rows beyond n holding NaN (poison = 1) or zeros, so that a read beyond n would stay inside the
// allocation and show in the result; the output is pre-filled with a sentinel byte and copied back whole, margins included.
#define TTS_RLG_KERNELS_ONLY
#include "../csrc/random_voice.h"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;

extern "C" {

enum { TTS_RLG_TEST_MARGIN = 4096, TTS_RLG_TEST_SENTINEL = 0xCB };
enum { TTS_RLG_TEST_LAYER = 0, TTS_RLG_TEST_NOISE = 1 };
enum { TTS_RLG_TEST_MAX_N = 64 }; // sized by the case matrix of tests/rlg_cases.py (2 * tile + 1 = 17)

// One case. Host pointers only. `out` holds TTS_RLG_TEST_MARGIN bytes, n * dim floats, TTS_RLG_TEST_MARGIN bytes.
//   LAYER  w [dim][dim], bias [dim], x [n][dim], act 0 | 1                  -> out f32 [n][dim]
//   NOISE  seeds [n] (64-bit), side 0 | 1                                   -> out f32 [n][dim]
struct tts_rlg_case {
  int op, dim, n, act, side, poison;
  const float *w, *bias, *x;
  const unsigned long long *seeds;
  void *out;
};

int tts_rlg_test_margin(void) { return TTS_RLG_TEST_MARGIN; }
int tts_rlg_test_tile(void) { return RLG_TILE; }
int tts_rlg_test_min_dim(void) { return RLG_MIN_DIM; }
int tts_rlg_test_max_dim(void) { return RLG_MAX_DIM; }
unsigned tts_rlg_test_tag(void) { return RLG_PHILOX_TAG; }

// 0 for a case that may run; hipErrorInvalidValue for a refused one
int tts_rlg_test_validate(const tts_rlg_case *c) {
  const int bad = (int)hipErrorInvalidValue;
  if (!c || !c->out) return bad;
  if (c->op != TTS_RLG_TEST_LAYER && c->op != TTS_RLG_TEST_NOISE) return bad;
  if (!rlg_dim_ok(c->dim)) return bad;
  if (c->n < 1 || c->n > TTS_RLG_TEST_MAX_N) return bad;
  if (c->poison != 0 && c->poison != 1) return bad;
  if (c->op == TTS_RLG_TEST_LAYER) {
    if (!c->w || !c->bias || !c->x) return bad;
    if (c->act != 0 && c->act != 1) return bad;
  } else {
    if (!c->seeds) return bad;
    if (c->side != 0 && c->side != 1) return bad;
  }
  return 0;
}

} // extern "C"

namespace {
struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_RLG_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_RLG_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_RLG_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h, size_t n) { return hipMemcpy(data(), h, n, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_RLG_TEST_MARGIN, hipMemcpyDeviceToHost); }
};
} // namespace

#define HT(x) do { hipError_t _e = (x); if (_e != hipSuccess) return (int)_e; } while (0)

extern "C" int tts_rlg_test_run(const tts_rlg_case *cp) {
  if (int rc = tts_rlg_test_validate(cp)) return rc;
  const tts_rlg_case &c = *cp;
  const size_t D = (size_t)c.dim, n = (size_t)c.n, tiles = (n + RLG_TILE - 1) / RLG_TILE;
  Dev w, b, x, seeds, out;
  HT(out.alloc(n * D * 4, TTS_RLG_TEST_SENTINEL));
  if (c.op == TTS_RLG_TEST_LAYER) {
    HT(w.alloc(D * D * 4, 0)); HT(w.put(c.w, D * D * 4));
    HT(b.alloc(D * 4, 0)); HT(b.put(c.bias, D * 4));
    HT(x.alloc(tiles * RLG_TILE * D * 4, c.poison ? 0xFF : 0)); HT(x.put(c.x, n * D * 4)); // whole tiles; the rows beyond n: NaN or zeros
  } else {
    HT(seeds.alloc(n * 8, 0)); HT(seeds.put(c.seeds, n * 8));
  }
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) {
    if (c.op == TTS_RLG_TEST_LAYER)
      e = rlg_launch_layer((const float *)w.data(), (const float *)b.data(), (const float *)x.data(), c.n, c.dim, c.act, (float *)out.data(), s);
    else
      e = rlg_launch_noise((const unsigned long long *)seeds.data(), (uint32_t)c.side, c.n, c.dim, (float *)out.data(), s);
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(out.get_all(c.out));
  return (int)(e != hipSuccess ? e : es);
}
