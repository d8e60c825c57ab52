// pcc_mlp_tiles_pop_d64.hip -- the population kernels of pcc_mlp_tiles_pop.h for observation lengths padded to 64, their three hidden
// classes: units of their own, so that the stand-alone kernels' units compile to what they always did.
#include "pcc_mlp_tiles_pop.h"

namespace pcc_tiles {
int launch_grad_pop_d64(const GradPopArgs &a, hipStream_t st, int *blocks_out) { return launch_d<64>(a, st, blocks_out); }
int launch_act_pop_d64(const ActPopArgs &a, hipStream_t st) { return launch_d<64>(a, st); }
}  // namespace pcc_tiles
