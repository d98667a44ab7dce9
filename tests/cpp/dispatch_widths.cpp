// The width dispatch of the SELL-family launchers (vexcl_amd/csrc/dispatch.hpp) on the host alone: no HIP, no library code.
// Every w in -1..40 through the range form (1..8 and 1..9) and the list form (3, 5, 7, 9); the booleans; one call of the callable per call.
#include <vexcl_amd/csrc/dispatch.hpp>

#include <cstdio>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s (line %d, w = %d)\n", #cond, __LINE__, w); ++failures; } } while (0)

template <int MAX> void range_form(int w) {
    int calls = 0, got = -1;
    vexhip::with_width<MAX>(w, [&](auto W) {
        static_assert(W() >= 0 && W() <= MAX, "a width outside 0..MAX was instantiated");
        ++calls; got = W();
    });
    CHECK(calls == 1);
    CHECK(got == (w >= 1 && w <= MAX ? w : 0));
}

int main() {
    for (int w = -1; w <= 40; ++w) {
        range_form<8>(w);
        range_form<9>(w);
        int calls = 0, got = -1;
        vexhip::with_width_of<3, 5, 7, 9>(w, [&](auto W) {
            static_assert(W() == 0 || W() == 3 || W() == 5 || W() == 7 || W() == 9, "a width outside the list was instantiated");
            ++calls; got = W();
        });
        CHECK(calls == 1);
        CHECK(got == (w == 3 || w == 5 || w == 7 || w == 9 ? w : 0));
        // a launcher without an any-width kernel: "not covered" is its own error
        bool covered = true;
        vexhip::with_width<8>(w, [&](auto W) { if constexpr (W() == 0) covered = false; });
        CHECK(covered == (w >= 1 && w <= 8));
    }
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const int w = 2 * a + b;
            int calls = 0, got = -1;
            vexhip::with_bool(a != 0, [&](auto A) { ++calls; got = A() ? 1 : 0; });
            CHECK(calls == 1 && got == a);
            calls = 0;
            vexhip::with_bools(a != 0, b != 0, [&](auto A, auto B) { ++calls; got = 2 * (A() ? 1 : 0) + (B() ? 1 : 0); });
            CHECK(calls == 1 && got == w);
        }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
