// pcc_mlp_tiles_d64.hip -- the tiled gradient and forward kernels of pcc_mlp_tiles.h for observation lengths padded to 64, their
// three hidden classes: a translation unit per length class, so that the classes compile side by side.
#include "pcc_mlp_tiles.h"

namespace pcc_tiles {
int launch_grad_d64(const GradArgs &a, hipStream_t st, int *blocks_out) { return launch_d<64>(a, st, blocks_out); }
int launch_act_d64(const ActArgs &a, hipStream_t st) { return launch_d<64>(a, st); }
}  // namespace pcc_tiles
