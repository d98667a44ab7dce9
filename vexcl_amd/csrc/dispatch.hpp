// Run-time values that are template arguments of a kernel, chosen in one place (no HIP header is needed here).  Each helper calls a generic
// lambda exactly once and hands it the value as a std::integral_constant / std::bool_constant, so that a launcher writes a kernel's
// argument list once:  with_width<8>(w, [&](auto W) { kernel<V, W()><<<grid, 256, 0, s>>>(...); });
// A width that is not covered arrives as 0 -- the kernels' any-width form; a launcher that has none says so with `if constexpr (W() == 0)`.
#pragma once
#include <type_traits>
#include <utility>

namespace vexhip {

// f(W) with W() == w where w is one of Ws..., W() == 0 otherwise
template <int... Ws, class F> inline void with_width_of(int w, F &&f) {
    const bool covered = ((w == Ws && (f(std::integral_constant<int, Ws>()), true)) || ...);
    if (!covered) f(std::integral_constant<int, 0>());
}

template <class F, int... Is> inline void with_width_seq(int w, F &&f, std::integer_sequence<int, Is...>) { with_width_of<(Is + 1)...>(w, f); }

// f(W) with W() == w for w in 1..MAX, W() == 0 otherwise
template <int MAX, class F> inline void with_width(int w, F &&f) { with_width_seq(w, f, std::make_integer_sequence<int, MAX>()); }

// f(B) and f(A, B): the booleans as std::bool_constants
template <class F> inline void with_bool(bool b, F &&f) {
    if (b) f(std::true_type()); else f(std::false_type());
}
template <class F> inline void with_bools(bool a, bool b, F &&f) {
    with_bool(a, [&](auto A) { with_bool(b, [&](auto B) { f(A, B); }); });
}

} // namespace vexhip
