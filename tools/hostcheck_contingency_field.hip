// Stand-alone check of the host path of wbx_contingency_field_partial in front of any launch: every refusal that returns before the
// device is touched, on a plan that lives in host memory.  Meant for a host sanitizer on a machine without a GPU:
//   cd weatherbenchx_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fno-gpu-rdc -I../../include \
//     -Xarch_host -fsanitize=address,undefined ../../tools/hostcheck_contingency_field.hip wbx_contingency_field.hip \
//     -o /tmp/hostcheck_contingency_field && /tmp/hostcheck_contingency_field
// Nothing is launched and no device is needed: the calls end at their argument checks.
#include <cstdio>
#include <cstring>

#include "../weatherbenchx_amd/csrc/wbx_common.hpp"

// (wbx_ctx.hip, where the library keeps its error text, brings the whole context with it: the buffer is stood in for here)
namespace wbx {
char* last_error_buf() {
  static thread_local char buf[512];
  return buf;
}
}  // namespace wbx

static int failures = 0;

static void expect(int rc, const char* what) {
  const char* msg = wbx::last_error_buf();
  if (rc != WBX_ERR_INVALID || strstr(msg, what) == nullptr) {
    printf("FAILED: wanted WBX_ERR_INVALID with '%s', got rc %d '%s'\n", what, rc, msg);
    ++failures;
  }
}

int main() {
  wbx_ctx ctx;
  wbx_s1_plan plan;
  memset(&plan, 0, sizeof(plan));
  plan.nkey = 2, plan.ndepth = 5, plan.nx = 65;
  plan.nchunk = 1, plan.depth_chunk = 5, plan.block_threads = 64, plan.vec = 1;
  double out[8];
  float p[1], t[1], c[1];
  uint8_t mask[1];
  auto call = [&](wbx_ctx* cx, const wbx_s1_plan* pl, int dtype, int thr_dtype, int nthr, int64_t stride, int64_t first, const void* pp,
                  const void* cc, const uint8_t* mm, double* oo) {
    return wbx_contingency_field_partial(cx, pl, dtype, thr_dtype, nthr, stride, first, pp, t, cc, mm, oo);
  };
  expect(call(nullptr, &plan, WBX_F32, WBX_F32, 1, 1, 0, p, c, nullptr, out), "ctx is NULL");
  expect(call(&ctx, nullptr, WBX_F32, WBX_F32, 1, 1, 0, p, c, nullptr, out), "plan is NULL");
  expect(call(&ctx, &plan, WBX_F32, WBX_F32, 0, 1, 0, p, c, nullptr, out), "thresholds per launch");
  expect(call(&ctx, &plan, WBX_F32, WBX_F32, WBX_CONT_MAX_THRESHOLDS + 1, 1, 0, p, c, nullptr, out), "thresholds per launch");
  expect(call(&ctx, &plan, 7, WBX_F32, 1, 1, 0, p, c, nullptr, out), "unknown dtype");
  expect(call(&ctx, &plan, WBX_F32, 7, 1, 1, 0, p, c, nullptr, out), "unknown thr_dtype");
  expect(call(&ctx, &plan, WBX_F32, WBX_F64, 2, 0, 0, p, c, nullptr, out), "thr_stride is 0");
  expect(call(&ctx, &plan, WBX_F32, WBX_F64, 2, 1, -1, p, c, nullptr, out), "thr_first is negative");
  expect(call(&ctx, &plan, WBX_F32, WBX_F32, 1, 1, 0, nullptr, c, nullptr, out), "p/t is NULL");
  expect(call(&ctx, &plan, WBX_F32, WBX_F32, 1, 1, 0, p, c, nullptr, nullptr), "partial_out is NULL");
  wbx_s1_plan bad = plan;
  bad.flags = WBX_FLAG_MASKED;
  expect(call(&ctx, &bad, WBX_F32, WBX_F32, 1, 1, 0, p, c, nullptr, out), "mask is NULL");
  bad.flags = WBX_FLAG_FAIR;
  expect(call(&ctx, &bad, WBX_F32, WBX_F32, 1, 1, 0, p, c, mask, out), "flags other than MASKED");
  bad = plan;
  bad.plane_rows = 5;
  expect(call(&ctx, &bad, WBX_F32, WBX_F32, 1, 1, 0, p, c, nullptr, out), "no plane mode");
  bad = plan;
  bad.depth_chunk = (int64_t)1 << 40;
  expect(call(&ctx, &bad, WBX_F32, WBX_F32, 1, 1, 0, p, c, nullptr, out), "2^32 or more points per partial");
  bad = plan;
  bad.vec = 3;
  expect(call(&ctx, &bad, WBX_F32, WBX_F32, 1, 1, 0, p, c, nullptr, out), "vec must be 1 or 4");
  printf(failures ? "%d check(s) failed\n" : "hostcheck_contingency_field: all refusals as documented (%d failed)\n", failures);
  return failures ? 1 : 0;
}
