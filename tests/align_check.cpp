// Unit cases of the host-side alignment helper (check_alignment in csrc/cgps_host.h), as a stand-alone program: built
// with hipcc and run by tests/test_memory_contract.py on a machine without a GPU (nothing here touches the runtime).
// Every address is inside a real buffer of this program; nothing is dereferenced.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "cgps_host.h"

namespace cgps_host {
thread_local char g_err[512] = "";
thread_local hipEvent_t g_prof_start = nullptr, g_prof_stop = nullptr;
}  // namespace cgps_host

using namespace cgps_host;

static int g_failed = 0;
#define CHECK(cond)                                         \
  do {                                                      \
    if (!(cond)) {                                          \
      ++g_failed;                                           \
      printf("FAIL line %d: %s [%s]\n", __LINE__, #cond, g_err); \
    }                                                       \
  } while (0)

int main() {
  alignas(512) static char buf[4096];
  char* base = buf;                       // 512-byte aligned
  CHECK(reinterpret_cast<uintptr_t>(base) % 512 == 0);
  // every boundary the contract names, met and missed by one byte, one element and one odd row
  CHECK(!misaligned(base, ALIGN_WS) && !misaligned(base, ALIGN_VEC) && !misaligned(base, 8) && !misaligned(base, 4));
  CHECK(misaligned(base + 1, 4) && misaligned(base + 4, 8) && misaligned(base + 8, ALIGN_VEC) && misaligned(base + 16, ALIGN_WS));
  CHECK(!misaligned(base + 16, ALIGN_VEC) && !misaligned(base + 256, ALIGN_WS) && misaligned(base + 128, ALIGN_WS));
  CHECK(!misaligned(nullptr, ALIGN_WS));                                    // null: somebody else's check
  CHECK(misaligned(base + 72, ALIGN_VEC));                                  // row 1 of 3 x 3 doubles
  CHECK(!misaligned(base + 144, ALIGN_VEC));                                // row 2 of them
  CHECK(misaligned(base + 4, ALIGN_VEC) && misaligned(base + 36, ALIGN_VEC) && misaligned(base + 100, ALIGN_VEC));   // fp32 d = 1, 3, 5
  CHECK(elem_bytes(CGPS_F32) == 4 && elem_bytes(CGPS_F64) == 8);

  // all fine: CGPS_OK and the message is left alone
  strcpy(g_err, "untouched");
  CHECK(check_alignment("entry", {{"Rs", base, ALIGN_VEC}, {"ws", base + 256, ALIGN_WS}, {"x", nullptr, ALIGN_VEC}, {"info", base + 4, 4}}) == CGPS_OK);
  CHECK(strcmp(g_err, "untouched") == 0);
  CHECK(check_alignment("entry", {}) == CGPS_OK);
  // the first offender is named, with the entry point and the boundary
  CHECK(check_alignment("cgps_solve", {{"Dp", base, ALIGN_VEC}, {"y", base + 72, ALIGN_VEC}, {"x", base + 8, ALIGN_VEC}}) == CGPS_ERR_ARG);
  CHECK(strstr(g_err, "cgps_solve: y = ") != nullptr && strstr(g_err, "16 bytes") != nullptr && strstr(g_err, " x ") == nullptr);
  CHECK(check_alignment("cgps_decompose", {{"Rs", base, ALIGN_VEC}, {"ws", base + 64, ALIGN_WS}}) == CGPS_ERR_ARG);
  CHECK(strstr(g_err, "cgps_decompose: ws = ") != nullptr && strstr(g_err, "256 bytes") != nullptr);
  CHECK(check_alignment("e", {{"out2", base + 4, 8}}) == CGPS_ERR_ARG && strstr(g_err, "out2") != nullptr);
  CHECK(check_alignment("e", {{"info", base + 2, 4}}) == CGPS_ERR_ARG && strstr(g_err, "info") != nullptr);
  printf("align_check: %d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
