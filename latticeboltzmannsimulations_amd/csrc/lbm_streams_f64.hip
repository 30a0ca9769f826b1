// lbm_streams_f64.hip -- explicit instantiations of the streaming kernel with the walls inside for a slab (k_stream_walls_slab), double (lbm_inst.hpp)
#define LBM_INST LBM_INST_STREAMS(double)
#include "lbm_inst.hpp"
