// General soft-argmax head family (head_any.hip): every cube side D with D % 4 == 0, 4 <= D <= 128.  The extern "C" launchers
// of head.hip send every size that the power-of-two family (D in {4,8,16,32,64}) does not take to these; same arguments,
// same outputs, same return codes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace xas {

size_t head_any_workspace_floats(int B, int K, int D);          // 0 + xas_last_error() when the size is refused
int head_any_fwd(const float* logits, int B, int K, int D, int num_hypo, int neighbor, float* kps, int64_t* z_idx,
                 float* depth_prob_map, int groups, float* stats, float* partial, void* stream);
int head_any_from_partials(const float* partial, int B, int K, int D, int nchunk, int num_hypo, int neighbor, float* kps,
                           int64_t* z_idx, float* depth_prob_map, int groups, float* stats, void* stream);
int head_any_bwd(const float* logits, const float* stats, const int64_t* z_idx, const float* grad_kps, int B, int K, int D,
                 int num_hypo, int neighbor, float* grad_logits, float* coef, float* amax_out, void* stream);

}  // namespace xas
