// precision_dispatch.h -- the precision code of a blocked tensor (dtype 0 = fp32, 1 = bf16, 2 = fp16) on the host: from the
// runtime code to the kernels' PREC template parameter, the validity check in front of it, and the channels one 16-byte slot
// holds.  Plain C++17 (only <type_traits>): the stand-alone test program compiles it without HIP.
#pragma once
#include <type_traits>

namespace srgan {

void set_error(const char* fmt, ...);                       // (common.h)
constexpr int PRECISION_EINVAL = -1;                         // = SRGAN_EINVAL (asserted where common.h is in sight: blocked16.h)

// Calls functor(std::integral_constant<int, CODE>{}) for the CODE of the list that equals dtype and returns true; a dtype that
// is not listed calls nothing and returns false.  Only the listed codes are instantiated: a family that has no fp32 kernels
// lists <1, 2>.
template <int... CODES, class Functor>
bool for_precision(int dtype, Functor&& functor) {
  return ((dtype == CODES ? (functor(std::integral_constant<int, CODES>{}), true) : false) || ...);
}

// The entry points' check in front of the dispatch: SRGAN_EINVAL with the caller's message for a code outside the list (an
// empty list accepts nothing: what a dispatch that found no kernel reports).
template <int... CODES>
int check_precision(int dtype, const char* message) {
  if (((dtype == CODES) || ...)) return 0;
  set_error("%s: requirement (dtype is one of the entry point's precision codes) failed", message);
  return PRECISION_EINVAL;
}

// Channels per 16-byte slot: four floats, or eight 16-bit values.
constexpr int slot_channels(int dtype) { return dtype == 0 ? 4 : 8; }
// Slots per pixel of a tensor of C channels.
constexpr int channel_groups(int C, int dtype) { return (C + slot_channels(dtype) - 1) / slot_channels(dtype); }

}  // namespace srgan
