// Born modelling, fused path on a bf16 forward-term store (3-D, fp32, O(8), stream kernel, standard form, sponge or no
// border; 4- and 8-row tiles, full and partial tiles): the IMAGE 3 variants of step3d_stream with q^n read as four bf16
// values per lane (ld_qf<true>) -- 22 B per point and step instead of 24.  Its own object: fwi_born3d.o and the stream
// objects keep their pinned kernel counts.
#include "fwi_stream3d.h"

namespace fwi {
template hipError_t launch_stream_born_bf16<4>(const GridDesc &, const StepArgs<float> &, const StreamTuning &, hipStream_t);
}  // namespace fwi
