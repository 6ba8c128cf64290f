// Kernel selection of the fusion stages: the calling thread's engine and one pure selector per stage. Each selector
// takes the engine as a parameter with the shape and alignment facts it needs and names the implementation to run;
// the C entries validate, select and switch. engine.cpp holds the selectors and the table they implement.
#pragma once
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "sagnn.h"

namespace sagnn {

enum class Engine { F16x2 = SAGNN_ENGINE_F16X2, F32 = SAGNN_ENGINE_F32, Valu = SAGNN_ENGINE_VALU };
Engine calling_engine();   // sagnn_set_engine of this thread; F16x2 on a thread that never set one

enum class LstmFwd { F16x2, F32Mfma, Split128, Valu };
enum class AttnFwd { Split, F32Mfma, Wide, Valu };
enum class AttnBwdFront { Split, F32Mfma, None };
enum class AttnBwdTail { F16x2, F32Mfma, None };
enum class LstmBwd { OneLaunch, SplitDw, None };   // SplitDw: BPTT without dW, then dW on the f16 engine (lstm_dw_f16)

// vec: x (and h_init) rows 16-byte aligned; h_vec: h too; drop_vec: the mask is absent or 16-byte aligned
LstmFwd select_lstm_fwd(Engine e, int d, int t, bool vec, int64_t ld_h, bool h_vec, bool train, bool drop, bool drop_vec);
AttnFwd select_attn_fwd(Engine e, int d, int t, int heads, bool vec);
AttnBwdFront select_attn_bwd_front(Engine e, int d, int t, int heads);
AttnBwdTail select_attn_bwd_tail(Engine e, int d);
LstmBwd select_lstm_bwd(Engine e, int d, bool workspace);

// Interval counts with a specialised attention kernel: the reference's configurations (graphNum 3..12) and the powers
// of two the weak-scaled benchmark produces. The fp32-MFMA forward takes any other t <= 32 in its run-time form.
using SpecialisedT = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 8, 12, 16>;
// The backward fronts that stop short of it (engine.cpp, "attn bwd front"): the pair form of the fp32-MFMA kernel, and
// at d = 128 the split kernel, where a pair's k / v / dk vectors take 144 of the 512 registers.
using MfmaBwdFrontT = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 8>;
using SplitBwdFrontT128 = std::integer_sequence<int, 1, 2, 3, 4, 5, 6>;

template <int... Ts>
constexpr bool has_t(int t, std::integer_sequence<int, Ts...>) {
  return (... || (t == Ts));
}
// Run-time t -> compile-time T: when t is in the sequence, sets rc = f(std::integral_constant<int, T>{}) for the T
// that equals t and returns true.
template <int... Ts, class F>
bool dispatch_t(int t, std::integer_sequence<int, Ts...>, F&& f, int& rc) {
  return (... || (t == Ts && (rc = f(std::integral_constant<int, Ts>{}), true)));
}

// shapes the kernel families cover; the launchers check them too
bool mhsa_split_supported(int d, int t, int heads);             // attn_split.hip, forward
bool attn_bwd_front_split_supported(int d, int t, int heads);   // attn_split.hip, backward front
bool mhsa_mfma_supported(int d, int t, int heads);              // fusion_mfma.hip
bool wide_supported(int d);                                     // fusion.hip, mhsa_mean_wide

}  // namespace sagnn
