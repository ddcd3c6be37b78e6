// loop_types.hpp -- the two plain types the loop-closure kernels (kernels_loop.hpp) share with the host optimisers (loop_optim.hpp).
#pragma once

namespace fls {

struct LoopMat4f { float m[16]; };  // column-major

struct NdtP2dPose {
    LoopMat4f T;
    double gauss_d1, gauss_d2;
    double j_ang[8][3];
    double h_ang[15][3];
};

}  // namespace fls
