// What the launches of the plane and grid products share on the host (plane.hpp, grid.hpp): the kernels' compile-time parameters chosen at
// run time, and the requirements of a one-launch step (halo.hpp).
#pragma once
#include "halo.hpp"
#include <type_traits>

namespace vexhip {
namespace {

// f(ZM, AUX), a generic lambda that launches kernel<.., ZM(), AUX(), ..>, with std::integral_constants for the addend form of the result (zm;
// plane.hip: 0 none, 1 an array, 2 x itself) and for the cache-policy immediate of the y stores (store_policy of a plan, VEXHIP_PLANE_STORE):
// 0 = non-temporal (2), 1 = non-temporal + sc1 (18), 2 = sc0 sc1 (17: write-through, the line leaves the L2: more of it is left for the halo
// lines of x), 3 = plain (0).  fp64 plane product at 512^3, tile 4 x 256: 0.395 / 0.393 / 0.384 / 0.387 ms; tile 2 x 512: 0.395 / 0.391 / 0.396 / 0.401.
template <class F> inline void with_launch_forms(int zm, int policy, F &&f) {
    auto with_aux = [&](auto ZM) {
        switch (policy) {
            case 1: f(ZM, std::integral_constant<int, 18>()); break;
            case 2: f(ZM, std::integral_constant<int, 17>()); break;
            case 3: f(ZM, std::integral_constant<int, 0>()); break;
            default: f(ZM, std::integral_constant<int, 2>());
        }
    };
    if (zm == 1) with_aux(std::integral_constant<int, 1>()); else if (zm == 2) with_aux(std::integral_constant<int, 2>()); else with_aux(std::integral_constant<int, 0>());
}

// a one-launch step over the planes [H.z0, H.z1) of a stored grid; pull_only: the launch has no push form (plane32.hip, grid.hip)
inline int check_halo_step(const halo_dev &H, int planes, long long plane_elements, bool pull_only) {
    VEXHIP_REQUIRE((pull_only ? H.pull != 0 : H.push_blocks >= 0) && H.z0 >= 0 && H.z1 > H.z0 && H.z1 <= planes && H.step && H.done && H.err, "bad halo step");
    VEXHIP_REQUIRE((long long)H.halo == plane_elements, "the ghost planes must be planes of the stored grid");
    VEXHIP_REQUIRE((!H.lo || H.z0 >= 1) && (!H.hi || H.z1 < planes), "a ghost plane outside the stored grid");
    return 0;
}

} // namespace
} // namespace vexhip
