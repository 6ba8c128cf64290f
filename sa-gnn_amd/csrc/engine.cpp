// Kernel selection of the fusion stages (engine.h). Every decision about which kernel a fusion call runs is made here.
//
// Rows are tried top to bottom; the first that holds is taken. "vec": x 16-byte aligned, ld_n and ld_t multiples of 4
// (and h_init likewise where given). "h aligned": h 16-byte aligned and ld_h a multiple of 4. Engine "any" includes VALU
// unless the row says otherwise.
//
// stage (entries)                   engine     taken when                                                  runs
// ---------------------------------------------------------------------------------------------------------------------
// LSTM fwd (lstm_fwd, _state,       valu       always                                                      Valu
//   _train, interval_fusion)        f16x2      d in {32, 64}, vec, h aligned, ld_h < 2^22, t*d < 2^18,     F16x2
//                                                not (training and a mask): inference takes the mask
//                                   f32,f16x2  d in {32, 64}, vec, h aligned                               F32Mfma
//                                   f16x2      d = 128, vec, ld_h % 4 = 0, h aligned; inference: no mask;   Split128
//                                                training: mask absent or aligned
//                                   any        otherwise                                                   Valu
// attention fwd (mhsa_mean,         valu       always (no wide path)                                       Valu
//   ln_mhsa_mean, interval_fusion)  f16x2      vec, heads = 16, d in {32, 64, 128}, t in {1..6, 8, 12, 16} Split
//                                   f32,f16x2  vec, d in {32, 64}, t <= 32, heads | d, d/heads a power of 2 F32Mfma
//                                   f32,f16x2  d % 32 = 0, 96 <= d <= 256                                  Wide (*)
//                                   any        otherwise                                                   Valu
// attn bwd front                    f16x2,valu heads = 16; d = 128 with t <= 6, d in {32, 64} with         Split
//                                                t in {1..6, 8, 12, 16}
//                                   any        d in {32, 64}, heads | d, d/heads in {2, 4}, t in {1..6, 8}  F32Mfma
//                                   any        otherwise                                                   None
// attn bwd tail                     f32        d in {32, 64}                                               F32Mfma
//                                   f16x2,valu d in {32, 64}                                               F16x2
// LSTM bwd (_ws)                    f16x2      d in {32, 64}, workspace given                              SplitDw
//                                   any        d in {32, 64}                                               OneLaunch
//
// (*) sagnn_mhsa_mean_f32 has no workspace and runs Valu instead. interval_fusion passes vec = true: its h is workspace.
// Workspace queries: sagnn_ln_mhsa_mean_workspace_bytes reserves nothing for Split / F32Mfma (vec assumed), y for
// Valu, y + Q|K|V for Wide; a caller with an unaligned x reserves y + Q|K|V itself (sagnn.h).
// sagnn_interval_fusion_workspace_bytes has no heads: it reserves h, plus Q|K|V wherever Wide is the fall-back of an
// unaligned call, so also where a fused kernel is taken (d = 128 under f16x2).
// VALU has no attention-backward kernels: the two _supported queries answer 0 under it, yet the _f32 entries run
// the f16x2 choice. The attention backward reads the engine of the thread it runs on (autograd: PyTorch's worker).
#include "engine.h"

#include "common.h"

namespace sagnn {

static thread_local Engine tl_engine = Engine::F16x2;
Engine calling_engine() { return tl_engine; }

static bool d32_or_64(int d) { return d == 32 || d == 64; }

LstmFwd select_lstm_fwd(Engine e, int d, int t, bool vec, int64_t ld_h, bool h_vec, bool train, bool drop, bool drop_vec) {
  if (e == Engine::Valu || !vec) return LstmFwd::Valu;
  if (d32_or_64(d)) {
    if (!h_vec) return LstmFwd::Valu;  // the f16 kernel stores h as 16-byte rows (raw_buffer_store_b128)
    // the f16 tile's rows are addressed with 32-bit byte offsets from a per-tile base (lstm_fwd_f16)
    if (e == Engine::F16x2 && !(train && drop) && ld_h < (1 << 22) && (int64_t)t * d < (1 << 18)) return LstmFwd::F16x2;
    return LstmFwd::F32Mfma;
  }
  if (d == 128 && e == Engine::F16x2 && h_vec && (train ? drop_vec : !drop)) return LstmFwd::Split128;
  return LstmFwd::Valu;
}

AttnFwd select_attn_fwd(Engine e, int d, int t, int heads, bool vec) {
  if (e == Engine::Valu) return AttnFwd::Valu;
  if (vec && e == Engine::F16x2 && mhsa_split_supported(d, t, heads)) return AttnFwd::Split;
  if (vec && mhsa_mfma_supported(d, t, heads)) return AttnFwd::F32Mfma;
  if (!d32_or_64(d) && wide_supported(d)) return AttnFwd::Wide;
  return AttnFwd::Valu;
}

AttnBwdFront select_attn_bwd_front(Engine e, int d, int t, int heads) {
  if (e != Engine::F32 && attn_bwd_front_split_supported(d, t, heads)) return AttnBwdFront::Split;
  if (mhsa_mfma_supported(d, t, heads) && (d / heads == 2 || d / heads == 4) && has_t(t, MfmaBwdFrontT{}))
    return AttnBwdFront::F32Mfma;
  return AttnBwdFront::None;
}

AttnBwdTail select_attn_bwd_tail(Engine e, int d) {
  return !d32_or_64(d) ? AttnBwdTail::None : e == Engine::F32 ? AttnBwdTail::F32Mfma : AttnBwdTail::F16x2;
}

LstmBwd select_lstm_bwd(Engine e, int d, bool workspace) {
  return !d32_or_64(d) ? LstmBwd::None : e == Engine::F16x2 && workspace ? LstmBwd::SplitDw : LstmBwd::OneLaunch;
}

bool mhsa_split_supported(int d, int t, int heads) {
  if (heads != 16 || !(d == 32 || d == 64 || d == 128)) return false;
  return has_t(t, SpecialisedT{});
}

// d = 32 / 64: every t of the forward; d = 128: t <= 6
bool attn_bwd_front_split_supported(int d, int t, int heads) {
  if (heads != 16) return false;
  return d == 128 ? has_t(t, SplitBwdFrontT128{}) : d32_or_64(d) && has_t(t, SpecialisedT{});
}

bool mhsa_mfma_supported(int d, int t, int heads) {
  if (!d32_or_64(d) || t < 1 || t > 32 || heads < 1 || d % heads) return false;
  const int dk = d / heads;
  return (dk & (dk - 1)) == 0;  // the per-head lane reduction needs a power of two
}

bool wide_supported(int d) { return d % 32 == 0 && d >= 32 && d <= 256; }

}  // namespace sagnn

extern "C" int sagnn_set_engine(int engine) {
  if (engine != SAGNN_ENGINE_F16X2 && engine != SAGNN_ENGINE_F32 && engine != SAGNN_ENGINE_VALU)
    return sagnn::fail(SAGNN_ERR_ARG, "sagnn_set_engine: unknown engine %d", engine);
  sagnn::tl_engine = static_cast<sagnn::Engine>(engine);
  return SAGNN_OK;
}
extern "C" int sagnn_get_engine(void) { return static_cast<int>(sagnn::calling_engine()); }
