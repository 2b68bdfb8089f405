// plan_driver.cpp — stand-alone driver of the tap-GEMM planner (vgen_amd/csrc/tapgemm_plan.cpp), linked with NOTHING else:
// no HIP, no libvgen_hip.so.  tests/test_tapgemm_plan.py builds the two files with the host compiler under
// -fsanitize=address,undefined and runs:   plan_driver rows.txt
// rows.txt: one launch per line, the 22 integers of tests/golden/make_plan_golden.py::FIELDS.  Every row is asked through
// the three entry points and compared with its recorded answer; then the plan table is walked through install, replace,
// empty (n = 0) and reset (n = -1), from heap buffers that are freed right after each call.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "vgen_hip.h"

void vgen_set_error(const char*, ...) {}   // the library's lives in cabi.cpp

namespace {

enum { DTYPE, MODE, M, N, C1, C2, TAPS, EPILOGUE, OUT_DTYPE, DUALW, SPLIT_OUT, LDO, LDR, ROWBIAS_LD, FLAGS, T_SHAPE, T_BN,
       T_SPLITK, SHAPE, BN, SPLITK, WS_BYTES, NFIELDS };
typedef std::vector<long long> Row;

alignas(16) char g_fake[16];   // a non-null aligned address: the planner never dereferences operands

vgen_tapgemm_args args_of(const Row& r) {
  vgen_tapgemm_args a;
  memset(&a, 0, sizeof(a));
  a.dtype = (int)r[DTYPE], a.mode = (int)r[MODE], a.M = r[M], a.N = (int)r[N], a.C1 = (int)r[C1], a.C2 = (int)r[C2];
  a.taps = (int)r[TAPS], a.epilogue = (int)r[EPILOGUE], a.out_dtype = (int)r[OUT_DTYPE], a.dualw = (int)r[DUALW];
  a.split_out = (int)r[SPLIT_OUT], a.ldo = r[LDO], a.ldr = r[LDR], a.rowbias_ld = r[ROWBIAS_LD];
  a.A = a.W = a.out = g_fake, a.lda = r[C1], a.lda2 = r[C2];
  if (r[C2]) a.A2 = g_fake;
  if (r[FLAGS] & 1) a.residual = (const float*)g_fake;
  if (r[FLAGS] & 2) a.rowbias = (const float*)g_fake, a.rows_per_rb = 1;
  if (r[FLAGS] & 4) a.colstats = (float*)g_fake;
  return a;
}

// the plan-table row keyed on `r`'s signature that asks for `plan`
void table_row(const Row& r, const long long plan[3], int64_t* out12) {
  const long long v[12] = {r[MODE], r[M], r[N], r[C1], r[C2], r[TAPS], r[EPILOGUE], r[OUT_DTYPE], r[FLAGS], plan[0], plan[1], plan[2]};
  for (int i = 0; i < 12; ++i) out12[i] = v[i];
}

// install `n` rows from a heap buffer that is gone when this returns
int install(const std::vector<int64_t>& rows, int n) {
  int64_t* heap = new int64_t[rows.size() + 1];
  for (size_t i = 0; i < rows.size(); ++i) heap[i] = rows[i];
  const int rc = vgen_tapgemm_set_plans(heap, n);
  memset(heap, 0x5a, sizeof(int64_t) * (rows.size() + 1));
  delete[] heap;
  return rc;
}

struct Answer {
  int32_t plan[3];
  size_t ws;
  bool operator==(const Answer& o) const { return !memcmp(plan, o.plan, sizeof(plan)) && ws == o.ws; }
};

bool ask(const Row& r, Answer* out) {
  const vgen_tapgemm_args a = args_of(r);
  if (vgen_tapgemm_query_plan(&a, out->plan) != 0) return false;
  out->ws = vgen_tapgemm_ws_bytes(&a);
  return true;
}

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "plan_driver: line %d: %s\n", __LINE__, #cond);      \
      return 1;                                                            \
    }                                                                      \
  } while (0)

}  // namespace

int main(int argc, char** argv) {
  CHECK(argc == 2);
  FILE* f = fopen(argv[1], "r");
  CHECK(f != nullptr);
  std::vector<Row> rows;
  for (;;) {
    Row r(NFIELDS);
    int got = 0;
    while (got < NFIELDS && fscanf(f, "%lld", &r[got]) == 1) ++got;
    if (got == 0) break;
    CHECK(got == NFIELDS);
    rows.push_back(r);
  }
  fclose(f);
  CHECK(!rows.empty());

  // every recorded launch, with its one-row table installed where the row has one
  const Row* walk = nullptr;
  for (const Row& r : rows) {
    if (r[T_SHAPE] >= 0) {
      std::vector<int64_t> t(12);
      table_row(r, &r[T_SHAPE], t.data());
      CHECK(install(t, 1) == 0);
    }
    Answer got;
    CHECK(ask(r, &got));
    if (r[T_SHAPE] >= 0) CHECK(vgen_tapgemm_set_plans(nullptr, -1) == 0);
    if (got.plan[0] != r[SHAPE] || got.plan[1] != r[BN] || got.plan[2] != r[SPLITK] || (long long)got.ws != r[WS_BYTES]) {
      fprintf(stderr, "plan_driver: M=%lld N=%lld C1=%lld: got (%d, %d, %d) ws %zu, recorded (%lld, %lld, %lld) ws %lld\n", r[M],
              r[N], r[C1], got.plan[0], got.plan[1], got.plan[2], got.ws, r[SHAPE], r[BN], r[SPLITK], r[WS_BYTES]);
      return 1;
    }
    if (!walk && r[T_SHAPE] >= 0 && r[SHAPE] == r[T_SHAPE] && r[BN] == r[T_BN] && r[SPLITK] == r[T_SPLITK]) walk = &r;
  }

  // the table's life cycle on a launch whose table row is honoured
  CHECK(walk != nullptr);
  const Row& w = *walk;
  Answer base, tabled, got;
  CHECK(ask(w, &base));                                   // compiled-in table
  std::vector<int64_t> two(24), one(12);
  Row other = w;
  other[M] += 1;                                          // a row that matches nothing asked here
  table_row(other, &w[T_SHAPE], two.data());
  table_row(w, &w[T_SHAPE], two.data() + 12);
  table_row(other, &w[T_SHAPE], one.data());
  CHECK(install(two, 2) == 0 && ask(w, &tabled));         // install: found in the second row
  CHECK(tabled.plan[0] == w[T_SHAPE] && tabled.plan[1] == w[T_BN] && tabled.plan[2] == w[T_SPLITK] && !(tabled == base));
  CHECK(install(one, 1) == 0 && ask(w, &got) && got == base);                  // replace: the old rows are gone
  CHECK(install(two, 2) == 0 && ask(w, &got) && got == tabled);
  CHECK(install(two, 0) == 0 && ask(w, &got) && got == base);                  // n = 0: an empty table
  CHECK(vgen_tapgemm_set_plans(nullptr, 0) == 0 && ask(w, &got) && got == base);
  CHECK(install(two, 2) == 0 && vgen_tapgemm_set_plans(nullptr, -1) == 0 && ask(w, &got) && got == base);   // reset
  CHECK(vgen_tapgemm_set_plans(nullptr, 1) == VGEN_E_BADARG && ask(w, &got) && got == base);
  CHECK(install(two, 2) == 0);                            // left installed: freed by the unit at exit, not leaked

  // the pre-check of the two queries
  vgen_tapgemm_args a = args_of(w);
  CHECK(vgen_tapgemm_query_plan(nullptr, got.plan) == VGEN_E_BADARG && vgen_tapgemm_query_plan(&a, nullptr) == VGEN_E_BADARG);
  CHECK(vgen_tapgemm_ws_bytes(nullptr) == 0);
  a.C1 = 96;
  CHECK(vgen_tapgemm_query_plan(&a, got.plan) == VGEN_E_BADARG && vgen_tapgemm_ws_bytes(&a) == 0);
  printf("%zu rows ok\n", rows.size());
  return 0;
}
