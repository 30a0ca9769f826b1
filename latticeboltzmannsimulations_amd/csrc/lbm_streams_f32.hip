// lbm_streams_f32.hip -- explicit instantiations of the streaming kernel with the walls inside for a slab (k_stream_walls_slab), float (lbm_inst.hpp)
#define LBM_INST LBM_INST_STREAMS(float)
#include "lbm_inst.hpp"
