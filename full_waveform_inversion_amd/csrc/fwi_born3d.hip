// Born modelling, fused path of the headline family (3-D, fp32, O(8), stream kernel, sponge or no border; standard and
// increment form, 4- and 8-row tiles, full and partial tiles): the scattering source w q^n joins q INSIDE step3d_stream
// (IMAGE 3) instead of being added by a second pass over the field (fwi_born.hip) -- 24 B per point and step (28 in
// increment form) instead of 32 (44).  Its own object: the stream objects keep their pinned kernel counts.
#include "fwi_stream3d.h"

namespace fwi {
template hipError_t launch_stream_born<float, 4>(const GridDesc &, const StepArgs<float> &, const StreamTuning &, hipStream_t);
}  // namespace fwi
