// norm_plan_driver.cpp — stand-alone driver of the norm planner (vgen_amd/csrc/norm_plan.cpp), linked with NOTHING else: no
// HIP, no libvgen_hip.so.  tests/test_norm_plan.py builds the two files with the host compiler under
// -fsanitize=address,undefined and runs:   norm_plan_driver rows.txt
// rows.txt: one shape per line, "G" + the 10 integers of tests/golden/make_norm_plan_golden.py::GN_FIELDS or "L" + the 6
// of LN_FIELDS.  Every row is asked through the query entries (and the workspace size) and compared with its recorded
// answer; then what the queries refuse.
#include <stdarg.h>
#include <stdio.h>

#include "vgen_hip.h"

static char g_err[256];
void vgen_set_error(const char* fmt, ...) {   // the library's lives in cabi.cpp
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define CHECK(cond)                                                             \
  do {                                                                          \
    if (!(cond)) {                                                              \
      fprintf(stderr, "norm_plan_driver: line %d: %s\n", __LINE__, #cond);      \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

int main(int argc, char** argv) {
  CHECK(argc == 2);
  FILE* f = fopen(argv[1], "r");
  CHECK(f != nullptr);
  size_t rows = 0;
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    long long r[10];
    const int n = kind == 'G' ? 10 : 6;
    CHECK(kind == 'G' || kind == 'L');
    for (int i = 0; i < n; ++i) CHECK(fscanf(f, "%lld", &r[i]) == 1);
    if (kind == 'G') {   // nb S C1 C2 has_cs | path nsplit rows_per lds_bytes ws_bytes
      int32_t got[4];
      CHECK(vgen_groupnorm_query_plan(r[0], r[1], (int32_t)r[2], (int32_t)r[3], 32, (int32_t)r[4], got) == 0);
      const size_t ws = vgen_groupnorm_ws_bytes(r[0], r[1]);
      if (got[0] != r[5] || got[1] != r[6] || got[2] != r[7] || got[3] != r[8] || (long long)ws != r[9]) {
        fprintf(stderr, "norm_plan_driver: nb=%lld S=%lld C=%lld+%lld cs=%lld: got (%d, %d, %d, %d) ws %zu, recorded (%lld, %lld, %lld, %lld) ws %lld\n",
                r[0], r[1], r[2], r[3], r[4], got[0], got[1], got[2], got[3], ws, r[5], r[6], r[7], r[8], r[9]);
        return 1;
      }
    } else {             // M d dtype | lpr ns grid
      int32_t got[3];
      CHECK(vgen_layernorm_query_plan(r[0], (int32_t)r[1], (int32_t)r[2], got) == 0);
      if (got[0] != r[3] || got[1] != r[4] || got[2] != r[5]) {
        fprintf(stderr, "norm_plan_driver: M=%lld d=%lld dtype=%lld: got (%d, %d, %d), recorded (%lld, %lld, %lld)\n", r[0], r[1],
                r[2], got[0], got[1], got[2], r[3], r[4], r[5]);
        return 1;
      }
    }
    ++rows;
  }
  fclose(f);
  CHECK(rows > 0);

  // what the queries refuse: a null output, and every size the launching entries refuse
  int32_t o[4];
  CHECK(vgen_groupnorm_query_plan(2, 1792, 320, 0, 32, 0, nullptr) == VGEN_E_BADARG);
  CHECK(vgen_groupnorm_query_plan(2, 1792, 320, 0, 7, 0, o) == VGEN_E_BADARG);
  CHECK(vgen_groupnorm_query_plan(2, 1792, 322, 0, 32, 0, o) == VGEN_E_BADARG);
  CHECK(vgen_groupnorm_query_plan(2, 1792, 2048, 2048, 32, 0, o) == VGEN_E_BADARG);
  CHECK(vgen_groupnorm_query_plan(0, 1792, 320, 0, 32, 0, o) == VGEN_E_BADARG);
  CHECK(vgen_groupnorm_query_plan(70000, 1792, 320, 0, 32, 0, o) == VGEN_E_BADARG);
  CHECK(vgen_groupnorm_query_plan(2, 1800, 320, 0, 32, 1, o) == VGEN_E_BADARG);
  CHECK(vgen_groupnorm_query_plan(65535, 1LL << 30, 3072, 0, 32, 0, o) == 0 && o[0] == 2 && o[1] == 1024);
  CHECK(vgen_layernorm_query_plan(64, 320, VGEN_F16, nullptr) == VGEN_E_BADARG);
  CHECK(vgen_layernorm_query_plan(64, 320, 5, o) == VGEN_E_BADARG);
  CHECK(vgen_layernorm_query_plan(64, 322, VGEN_F16, o) == VGEN_E_BADARG);
  CHECK(vgen_layernorm_query_plan(1LL << 33, 320, VGEN_F16, o) == VGEN_E_BADARG);
  CHECK(vgen_layernorm_query_plan((1LL << 32) - 1, 64, VGEN_F32, o) == 0 && o[0] == 16 && o[1] == 0 && o[2] == (1 << 28));
  CHECK(vgen_layernorm_query_plan(0, 320, VGEN_F16, o) == 0 && o[2] == 0);
  printf("%zu rows ok\n", rows);
  return 0;
}
