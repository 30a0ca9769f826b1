// lbm_streamw_f64.hip -- explicit instantiations of the streaming kernel with the walls inside (k_stream_walls), double (lbm_inst.hpp)
#define LBM_INST LBM_INST_STREAMW(double)
#include "lbm_inst.hpp"
