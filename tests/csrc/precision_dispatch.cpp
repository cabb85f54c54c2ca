// Stand-alone driver of sr-gan_amd/csrc/precision_dispatch.h for tests/test_precision_dispatch_cpu.py: the header alone, no
// HIP.  It prints what the header did, one record per line; the test holds the expectations.
//   dispatch <list> <dtype> <returned> <calls> <constant seen, -99 if none>
//   check <list> <dtype> <status> <message recorded through set_error, - if none>
//   slot_channels <dtype> <value>
//   channel_groups <C> <dtype> <value>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "precision_dispatch.h"

static std::string g_error;

namespace srgan {
void set_error(const char* fmt, ...) {
  char text[512];
  va_list arguments;
  va_start(arguments, fmt);
  vsnprintf(text, sizeof(text), fmt, arguments);
  va_end(arguments);
  g_error = text;
}
}  // namespace srgan

// the constants are compile-time values: a kernel's template argument
template <int PREC> struct Kernel { static constexpr int code = PREC; };
static_assert(srgan::slot_channels(0) == 4 && srgan::slot_channels(1) == 8 && srgan::slot_channels(2) == 8, "constexpr");
static_assert(srgan::channel_groups(9, 0) == 3 && srgan::channel_groups(9, 2) == 2, "constexpr");

template <int... CODES>
static void run(const char* list) {
  for (int dtype = -1; dtype <= 3; ++dtype) {
    int calls = 0, seen = -99;
    const bool returned = srgan::for_precision<CODES...>(dtype, [&](auto prec) {
      ++calls;
      seen = Kernel<decltype(prec)::value>::code;
    });
    printf("dispatch %s %d %d %d %d\n", list, dtype, returned ? 1 : 0, calls, seen);
    g_error.clear();
    const int status = srgan::check_precision<CODES...>(dtype, "the caller's message");
    printf("check %s %d %d %s\n", list, dtype, status, g_error.empty() ? "-" : g_error.c_str());
  }
}

int main() {
  run<0, 1, 2>("0,1,2");
  run<1, 2>("1,2");
  run<>("none");
  for (int dtype = 0; dtype <= 2; ++dtype) {
    printf("slot_channels %d %d\n", dtype, srgan::slot_channels(dtype));
    for (int C : {1, 4, 5, 8, 9}) printf("channel_groups %d %d %d\n", C, dtype, srgan::channel_groups(C, dtype));
  }
  return 0;
}
