// lbm_streamw_f32.hip -- explicit instantiations of the streaming kernel with the walls inside (k_stream_walls), float (lbm_inst.hpp)
#define LBM_INST LBM_INST_STREAMW(float)
#include "lbm_inst.hpp"
