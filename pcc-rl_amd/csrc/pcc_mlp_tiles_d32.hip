// pcc_mlp_tiles_d32.hip -- the tiled gradient and forward kernels of pcc_mlp_tiles.h for observation lengths padded to 32, their
// three hidden classes: a translation unit per length class, so that the classes compile side by side.
#include "pcc_mlp_tiles.h"

namespace pcc_tiles {
int launch_grad_d32(const GradArgs &a, hipStream_t st, int *blocks_out) { return launch_d<32>(a, st, blocks_out); }
int launch_act_d32(const ActArgs &a, hipStream_t st) { return launch_d<32>(a, st); }
}  // namespace pcc_tiles
