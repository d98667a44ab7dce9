// GPU: vex::SpMat and vex::sparse::* against a host recomputation, as the
// reference's tests/spmv.cpp:10-260 and tests/sparse_matrices.cpp:66-237 do,
// on the 2-"device" context (partitioning + ghost exchange are exercised).
#include <cstdlib>
#include <array>
#include <cstring>
#include "vex_test.hpp"

template <class R, class C>
std::vector<double> host_spmv(const std::vector<R> &row, const std::vector<C> &col, const std::vector<double> &val,
        const std::vector<double> &x) {
    std::vector<double> y(row.size() - 1);
    for (size_t i = 0; i + 1 < row.size(); ++i) {                  // tests/spmv.cpp:28-32
        double s = 0;
        for (size_t j = row[i]; j < row[i + 1]; ++j) s += val[j] * x[col[j]];
        y[i] = s;
    }
    return y;
}

TEST_CASE(spmv_square_multi_device) {                                // spmv.cpp:10-59
    const size_t n = 1024;
    std::vector<size_t> row, col; std::vector<double> val;
    random_matrix(n, n, 16, row, col, val);
    std::vector<double> x = random_vector<double>(n);
    auto want = host_spmv(row, col, val, x);
    vex::SpMat<double> A(ctx, n, n, row.data(), col.data(), val.data());
    CHECK(A.rows() == n && A.cols() == n && A.nonzeros() == val.size());
    vex::vector<double> X(ctx, x), Y(ctx, n);
    Y = A * X;
    check_sample(Y, [&](size_t i, double v) { CHECK_CLOSE(v, want[i], 1e-8); });
    Y = A * X; Y -= A * X;
    check_sample(Y, [&](size_t, double v) { CHECK_SMALL(v, 1e-8); });
    Y = 1; Y += 42 * (A * X);
    check_sample(Y, [&](size_t i, double v) { CHECK_CLOSE(v, 1 + 42 * want[i], 1e-8); });
    Y = X + A * X;
    check_sample(Y, [&](size_t i, double v) { CHECK_CLOSE(v, x[i] + want[i], 1e-8); });
    Y = X - 2 * (A * X) + A * X;
    check_sample(Y, [&](size_t i, double v) { CHECK_CLOSE(v, x[i] - want[i], 1e-7); });
    Y = -(A * X);
    check_sample(Y, [&](size_t i, double v) { CHECK_CLOSE(v, -want[i], 1e-8); });
    // every row, not a sample
    Y = A * X;
    std::vector<double> got(n); vex::copy(Y, got);
    for (size_t i = 0; i < n; ++i) CHECK_CLOSE(got[i], want[i], 1e-8);
}

TEST_CASE(spmv_back_to_back_products_without_host_sync) {
    // y = A*x; x = A*y; ... with no host synchronisation in between and a matrix whose first partition does far more
    // work than the second: the next product's ghost exchange must not overwrite the ghost buffer the slower device
    // is still reading (the reference fences with finish() at the top of every apply, spmat.hpp:125-128), nor repack
    // a send buffer that is still being shipped.  A banded matrix with wide coupling across the partition boundary.
    const size_t n = 1 << 16;
    std::vector<size_t> row(1, 0), col; std::vector<double> val;
    for (size_t i = 0; i < n; ++i) {
        const int per_side = i < n / 2 ? 40 : 1;                      // device 0 is the slow one
        for (int k = -per_side; k <= per_side; ++k) {
            long c = (long)i + 97l * k;
            if (c < 0 || c >= (long)n) continue;
            col.push_back((size_t)c); val.push_back(1.0 / (1 + std::abs(k)) / (2 * per_side + 1));
        }
        row.push_back(col.size());
    }
    std::vector<double> x = random_vector<double>(n), a = x, b(n);
    const int steps = 24;
    for (int s = 0; s < steps; ++s) { b = host_spmv(row, col, val, a); a.swap(b); }
    vex::SpMat<double> A(ctx, n, n, row.data(), col.data(), val.data());
    vex::vector<double> X(ctx, x), Y(ctx, n);
    for (int s = 0; s < steps; s += 2) { Y = A * X; X = A * Y; }      // no finish() anywhere
    std::vector<double> got(n); vex::copy(X, got);
    double worst = 0;
    for (size_t i = 0; i < n; ++i) worst = std::max(worst, std::fabs(got[i] - a[i]) / (std::fabs(a[i]) + 1e-300));
    CHECK(worst < 1e-10);
}

TEST_CASE(spmv_from_device_arrays) {
    // vex::SpMat built from DEVICE CSR arrays (no host staging) == the host-array constructor, bit for bit
    const size_t n = 40, N = n * n * n;
    std::vector<int> row(1, 0), col; std::vector<double> val;
    for (size_t k = 0, idx = 0; k < n; ++k) for (size_t j = 0; j < n; ++j) for (size_t i = 0; i < n; ++i, ++idx) {
        if (i == 0 || i == n - 1 || j == 0 || j == n - 1 || k == 0 || k == n - 1) { col.push_back((int)idx); val.push_back(1); }
        else for (long d : {-(long)(n * n), -(long)n, -1l, 0l, 1l, (long)n, (long)(n * n)}) { col.push_back((int)(idx + d)); val.push_back(d ? -0.25 * (1 + (idx + (d > 0 ? d : 0)) % 7) : 6.5); }
        row.push_back((int)col.size());
    }
    std::vector<vex::backend::command_queue> q1(1, ctx.queue(0));
    vex::SpMat<double, int, int> H(q1, N, N, row.data(), col.data(), val.data());
    vex::backend::device_vector<int> dr(q1[0], row.size(), row.data()), dc(q1[0], col.size(), col.data());
    vex::backend::device_vector<double> dv(q1[0], val.size(), val.data());
    vex::SpMat<double, int, int> D(q1, N, N, col.size(), dr, dc, dv);
    CHECK(D.rows() == N && D.nonzeros() == col.size());
    CHECK(D.storage_info().format == H.storage_info().format && D.storage_info().format == VEXHIP_SPMAT_SELL8V);   // 7 diagonals, 9 distinct values
    std::vector<double> x = random_vector<double>(N), yh(N), yd(N);
    vex::vector<double> X(q1, x), Y(q1, N);
    Y = H * X; vex::copy(Y, yh);
    Y = D * X; vex::copy(Y, yd);
    bool same = true;
    for (size_t i = 0; i < N; ++i) same = same && yh[i] == yd[i];
    CHECK(same);
    std::vector<size_t> r2(row.begin(), row.end()), c2(col.begin(), col.end());
    auto want = host_spmv(r2, c2, val, x);
    for (size_t i = 0; i < N; i += 97) CHECK_CLOSE(yd[i], want[i], 1e-8);
}

TEST_CASE(spmv_from_device_strips_multi_device) {
    // round 4: vex::SpMat on a MULTI-device context built from one DEVICE strip per device (strip-local row pointers, global
    // columns; nothing staged through the host, every device splits and converts its own strip, all at once) == the
    // host-array constructor on the same context, bit for bit: the same split, the same storages, the same exchange
    // (spmat.hpp:71-106 builds from host arrays only)
    const size_t n = 36, N = n * n * n;
    std::vector<int> row(1, 0), col; std::vector<double> val;
    for (size_t k = 0, idx = 0; k < n; ++k) for (size_t j = 0; j < n; ++j) for (size_t i = 0; i < n; ++i, ++idx) {
        if (i == 0 || i == n - 1 || j == 0 || j == n - 1 || k == 0 || k == n - 1) { col.push_back((int)idx); val.push_back(1); }
        else for (long d : {-(long)(n * n), -(long)n, -1l, 0l, 1l, (long)n, (long)(n * n)}) { col.push_back((int)(idx + d)); val.push_back(d ? -0.25 * (1 + (idx + (d > 0 ? d : 0)) % 7) : 6.5); }
        row.push_back((int)col.size());
    }
    const std::vector<vex::backend::command_queue> &q = ctx.queue();
    const std::vector<size_t> part = vex::partition(N, q);
    vex::SpMat<double, int, int> H(q, N, N, row.data(), col.data(), val.data());
    std::vector<vex::backend::device_vector<int>> dr(q.size()), dc(q.size());
    std::vector<vex::backend::device_vector<double>> dv(q.size());
    std::vector<size_t> snz(q.size());
    for (unsigned d = 0; d < q.size(); ++d) {
        const size_t r0 = part[d], r1 = part[d + 1], first = (size_t)row[r0];
        snz[d] = (size_t)row[r1] - first;
        std::vector<int> sp(r1 - r0 + 1);
        for (size_t i = 0; i <= r1 - r0; ++i) sp[i] = row[r0 + i] - (int)first;
        dr[d] = vex::backend::device_vector<int>(q[d], sp.size(), sp.data());
        dc[d] = vex::backend::device_vector<int>(q[d], std::max<size_t>(1, snz[d]), col.data() + first);
        dv[d] = vex::backend::device_vector<double>(q[d], std::max<size_t>(1, snz[d]), val.data() + first);
    }
    vex::SpMat<double, int, int> D(q, N, N, dr, dc, dv, snz);
    CHECK(D.rows() == N && D.cols() == N && D.nonzeros() == col.size());
    for (unsigned d = 0; d < q.size(); ++d) CHECK(D.storage_info(d).format == H.storage_info(d).format);
    std::vector<double> x = random_vector<double>(N), yh(N), yd(N);
    vex::vector<double> X(ctx, x), Y(ctx, N);
    Y = H * X; vex::copy(Y, yh);
    Y = D * X; vex::copy(Y, yd);
    bool same = true;
    for (size_t i = 0; i < N; ++i) same = same && yh[i] == yd[i];
    CHECK(same);
    Y = X; Y += 2.5 * (D * X); vex::copy(Y, yd);          // and through the additive machinery
    std::vector<size_t> r2(row.begin(), row.end()), c2(col.begin(), col.end());
    auto want = host_spmv(r2, c2, val, x);
    for (size_t i = 0; i < N; i += 89) CHECK_CLOSE(yd[i], x[i] + 2.5 * want[i], 1e-8);
    // the timed form of the product reports a phase table per device and leaves the same y
    std::vector<std::array<float, 4>> ms;
    D.apply_timed(X, Y, ms);
    CHECK(ms.size() == q.size());
    for (const auto &m : ms) CHECK(m[0] > 0 && m[1] >= 0 && m[2] >= 0 && m[3] >= 0);
    vex::copy(Y, yd);
    same = true;
    for (size_t i = 0; i < N; ++i) same = same && yh[i] == yd[i];
    CHECK(same);
}

TEST_CASE(spmv_one_launch_step_multi_device) {
    // round 6: a plane partition of a 7-point operator on 512-point lines -- the headline's shape -- on a multi-device context: every
    // device's product is ONE launch on its strip stored with its two ghost planes, the neighbours' boundary planes of x read in place
    // (vexcl/spmat.hpp setup_halo; reference: the five phases of spmat.hpp:120-185).  The bits must be those of the same matrix on
    // ONE device (a row's entries stay in column order), for '=', '+=' and a scaled product, from host arrays and from device strips.
    const std::vector<vex::backend::command_queue> &q = ctx.queue();
    if (q.size() < 2) return;
    const size_t nx = 512, ny = 16, nz = 8 * q.size(), N = nx * ny * nz, P = nx * ny;
    std::vector<int> row(1, 0), col; std::vector<double> val;
    for (size_t k = 0, idx = 0; k < nz; ++k) for (size_t j = 0; j < ny; ++j) for (size_t i = 0; i < nx; ++i, ++idx) {
        if (i == 0 || i == nx - 1 || j == 0 || j == ny - 1 || k == 0 || k == nz - 1) { col.push_back((int)idx); val.push_back(1); }
        else for (long d : {-(long)P, -(long)nx, -1l, 0l, 1l, (long)nx, (long)P}) { col.push_back((int)(idx + d)); val.push_back(d ? -0.25 * (d > 0 ? 3 : 1) : 6.5); }
        row.push_back((int)col.size());
    }
    const std::vector<size_t> part = vex::partition(N, q);
    for (unsigned d = 0; d < q.size(); ++d) CHECK((part[d + 1] - part[d]) % P == 0);
    // (a grid this small has too many boundary lines for the plane plan's liking -- more than one line in 16 off the hot block:
    //  the plan is forced, as in the Python tests of the plane product)
    setenv("VEXHIP_PLANE_FORCE", "1", 1);
    struct unforce { ~unforce() { unsetenv("VEXHIP_PLANE_FORCE"); } } unforce_at_exit;
    vex::SpMat<double, int, int> A(q, N, N, row.data(), col.data(), val.data());
    CHECK(std::string(A.step_kind()).find("one launch per device") == 0);
    if (std::string(A.step_kind()).find("one launch per device") != 0) std::cerr << "one-launch step declined: " << A.halo_declined() << std::endl;
    for (unsigned d = 0; d < q.size(); ++d) CHECK(A.storage_info(d).plane.usable == 1);
    // the same matrix on one device
    std::vector<vex::backend::command_queue> q1(1, q[0]);
    vex::SpMat<double, int, int> A1(q1, N, N, row.data(), col.data(), val.data());
    std::vector<double> x = random_vector<double>(N), y1(N), ym(N);
    vex::vector<double> X(ctx, x), Y(ctx, N), X1(q1, x), Y1(q1, N);
    auto same_bits = [&]() { vex::copy(Y, ym); vex::copy(Y1, y1); for (size_t i = 0; i < N; ++i) if (std::memcmp(&ym[i], &y1[i], 8)) return false; return true; };
    Y = A * X; Y1 = A1 * X1;
    CHECK(same_bits());
    for (int rep = 0; rep < 20; ++rep) { Y = A * X; X = 0.5 * X + 0.25; Y += 1.5 * (A * X); X1 = 0.5 * X1 + 0.25; }     // x rewritten between products: the ordering of the streams is what is tested
    Y1 = A1 * X1; Y = A * X;
    CHECK(same_bits());
    Y = X; Y += 2.5 * (A * X); Y -= A * X; Y1 = X1; Y1 += 2.5 * (A1 * X1); Y1 -= A1 * X1;
    CHECK(same_bits());
    std::vector<size_t> r2(row.begin(), row.end()), c2(col.begin(), col.end());
    vex::copy(X, x);
    auto want = host_spmv(r2, c2, val, x);
    Y = A * X; vex::copy(Y, ym);
    for (size_t i = 0; i < N; i += 53) CHECK_CLOSE(ym[i], want[i], 1e-8);
    // from device strips
    std::vector<vex::backend::device_vector<int>> dr(q.size()), dc(q.size());
    std::vector<vex::backend::device_vector<double>> dv(q.size());
    std::vector<size_t> snz(q.size());
    for (unsigned d = 0; d < q.size(); ++d) {
        const size_t r0 = part[d], r1 = part[d + 1], first = (size_t)row[r0];
        snz[d] = (size_t)row[r1] - first;
        std::vector<int> sp(r1 - r0 + 1);
        for (size_t i = 0; i <= r1 - r0; ++i) sp[i] = row[r0 + i] - (int)first;
        dr[d] = vex::backend::device_vector<int>(q[d], sp.size(), sp.data());
        dc[d] = vex::backend::device_vector<int>(q[d], std::max<size_t>(1, snz[d]), col.data() + first);
        dv[d] = vex::backend::device_vector<double>(q[d], std::max<size_t>(1, snz[d]), val.data() + first);
    }
    vex::SpMat<double, int, int> D(q, N, N, dr, dc, dv, snz);
    CHECK(std::string(D.step_kind()).find("one launch per device") == 0);
    Y = D * X; Y1 = A1 * X1;
    CHECK(same_bits());
    std::vector<std::array<float, 4>> ms;
    D.apply_timed(X, Y, ms);
    CHECK(ms.size() == q.size());
    CHECK(same_bits());
    // float on 512-point lines (plane32.hip) and double on lines of another length (the grid product): the same step
    {
        std::vector<float> valf(val.begin(), val.end()), xf(x.begin(), x.end()), yf(N), yf1(N);
        vex::SpMat<float, int, int> F(q, N, N, row.data(), col.data(), valf.data()), F1(q1, N, N, row.data(), col.data(), valf.data());
        CHECK(std::string(F.step_kind()).find("one launch per device") == 0);
        if (std::string(F.step_kind()).find("one launch per device") != 0) std::cerr << "float: one-launch step declined: " << F.halo_declined() << std::endl;
        vex::vector<float> XF(ctx, xf), YF(ctx, N), XF1(q1, xf), YF1(q1, N);
        YF = F * XF; YF1 = F1 * XF1;
        YF += 0.5f * (F * XF); YF1 += 0.5f * (F1 * XF1);
        vex::copy(YF, yf); vex::copy(YF1, yf1);
        bool same = true;
        for (size_t i = 0; i < N; ++i) same = same && std::memcmp(&yf[i], &yf1[i], 4) == 0;
        CHECK(same);
    }
    {
        const size_t gx = 96, gy = 12, gz = 8 * q.size(), GN = gx * gy * gz, GP = gx * gy;
        std::vector<int> grow(1, 0), gcol; std::vector<double> gval;
        for (size_t k = 0, idx = 0; k < gz; ++k) for (size_t j = 0; j < gy; ++j) for (size_t i = 0; i < gx; ++i, ++idx) {
            if (i == 0 || i == gx - 1 || j == 0 || j == gy - 1 || k == 0 || k == gz - 1) { gcol.push_back((int)idx); gval.push_back(1); }
            else for (long d : {-(long)GP, -(long)gx, -1l, 0l, 1l, (long)gx, (long)GP}) { gcol.push_back((int)(idx + d)); gval.push_back(d ? -0.5 * (d > 0 ? 3 : 1) : 7.5); }
            grow.push_back((int)gcol.size());
        }
        const std::vector<size_t> gpart = vex::partition(GN, q);
        bool whole = true;
        for (unsigned d = 0; d < q.size(); ++d) whole = whole && (gpart[d + 1] - gpart[d]) % GP == 0;
        if (whole) {
            vex::SpMat<double, int, int> G(q, GN, GN, grow.data(), gcol.data(), gval.data()), G1(q1, GN, GN, grow.data(), gcol.data(), gval.data());
            CHECK(std::string(G.step_kind()).find("one launch per device") == 0);
            if (std::string(G.step_kind()).find("one launch per device") != 0) std::cerr << "96-point lines: one-launch step declined: " << G.halo_declined() << std::endl;
            std::vector<double> gx0 = random_vector<double>(GN), ga(GN), gb(GN);
            vex::vector<double> GX(ctx, gx0), GY(ctx, GN), GX1(q1, gx0), GY1(q1, GN);
            GY = G * GX; GY1 = G1 * GX1;
            for (int rep = 0; rep < 5; ++rep) { GX = 0.5 * GX + 0.25; GY += 1.5 * (G * GX); GX1 = 0.5 * GX1 + 0.25; GY1 += 1.5 * (G1 * GX1); }
            vex::copy(GY, ga); vex::copy(GY1, gb);
            bool same = true;
            for (size_t i = 0; i < GN; ++i) same = same && std::memcmp(&ga[i], &gb[i], 8) == 0;
            CHECK(same);
        }
    }
    // a general matrix on the same context keeps the exchange, and says why
    {
        const size_t n = 1024;
        std::vector<size_t> rr; std::vector<int> cc; std::vector<double> vv;
        random_matrix(n, n, 16, rr, cc, vv);
        vex::SpMat<double, int> G(ctx, n, n, rr.data(), cc.data(), vv.data());
        CHECK(std::string(G.step_kind()) == "pack / exchange / local / remote" && !G.halo_declined().empty());
    }
}

TEST_CASE(spmv_one_launch_step_general_matrix_multi_device) {
    // round 6: the one-launch step for ANY strip stored with diagonal codes (csrc/sell8.hip, the pair product's role): a 7-point pattern with a
    // different value in every entry (nothing to code: SELL8, values in the slices) and a banded matrix with an odd diagonal whose pairs
    // straddle the seam between a ghost range and the device's rows.  Bits of the same matrix on one device; '=', '+=', scaled, x rewritten.
    const std::vector<vex::backend::command_queue> &q = ctx.queue();
    if (q.size() < 2) return;
    const size_t nx = 64, ny = 32, nz = 16 * q.size(), N = nx * ny * nz, P = nx * ny;      // a plane = 2048 rows = 4 slices; strips of 16 planes
    for (int kind = 0; kind < 2; ++kind) {
        std::vector<int> row(1, 0), col; std::vector<double> val;
        for (size_t k = 0, idx = 0; k < nz; ++k) for (size_t j = 0; j < ny; ++j) for (size_t i = 0; i < nx; ++i, ++idx) {
            const bool inner = i > 0 && i + 1 < nx && j > 0 && j + 1 < ny && k > 0 && k + 1 < nz;
            if (!inner) { col.push_back((int)idx); val.push_back(1); }
            else if (kind == 0) for (long d : {-(long)P, -(long)nx, -1l, 0l, 1l, (long)nx, (long)P}) { col.push_back((int)(idx + d)); val.push_back(1.0 + 1e-3 * (double)((idx * 7 + (size_t)(d + (long)P)) % 9973)); }
            else for (long d : {-(long)P + 1, -3l, 0l, 5l, (long)P - 1}) { col.push_back((int)(idx + d)); val.push_back(0.5 + 1e-3 * (double)((idx * 5 + (size_t)(d + (long)P)) % 7919)); }
            row.push_back((int)col.size());
        }
        const std::vector<size_t> part = vex::partition(N, q);
        for (unsigned d = 0; d < q.size(); ++d) CHECK((part[d + 1] - part[d]) % P == 0);
        vex::SpMat<double, int, int> A(q, N, N, row.data(), col.data(), val.data());
        CHECK(std::string(A.step_kind()).find("one launch per device") == 0);
        if (std::string(A.step_kind()).find("one launch per device") != 0) std::cerr << "one-launch step declined: " << A.halo_declined() << std::endl;
        for (unsigned d = 0; d < q.size(); ++d) CHECK(A.storage_info(d).format == VEXHIP_SPMAT_SELL8 && !A.storage_info(d).plane.usable && !A.storage_info(d).grid.usable);
        std::vector<vex::backend::command_queue> q1(1, q[0]);
        vex::SpMat<double, int, int> A1(q1, N, N, row.data(), col.data(), val.data());
        std::vector<double> x = random_vector<double>(N), y1(N), ym(N);
        vex::vector<double> X(ctx, x), Y(ctx, N), X1(q1, x), Y1(q1, N);
        auto same_bits = [&]() { vex::copy(Y, ym); vex::copy(Y1, y1); for (size_t i = 0; i < N; ++i) if (std::memcmp(&ym[i], &y1[i], 8)) return false; return true; };
        Y = A * X; Y1 = A1 * X1;
        CHECK(same_bits());
        for (int rep = 0; rep < 20; ++rep) { Y = A * X; X = 0.5 * X + 0.25; Y += 1.5 * (A * X); X1 = 0.5 * X1 + 0.25; }
        Y1 = A1 * X1; Y = A * X;
        CHECK(same_bits());
        Y = X; Y += 2.5 * (A * X); Y -= A * X; Y1 = X1; Y1 += 2.5 * (A1 * X1); Y1 -= A1 * X1;
        CHECK(same_bits());
        std::vector<size_t> r2(row.begin(), row.end()), c2(col.begin(), col.end());
        vex::copy(X, x);
        auto want = host_spmv(r2, c2, val, x);
        Y = A * X; vex::copy(Y, ym);
        for (size_t i = 0; i < N; i += 53) CHECK_CLOSE(ym[i], want[i], 1e-8);
    }
}

TEST_CASE(spmv_one_launch_step_two_dimensional_multi_device) {
    // round 6: a 5-point operator on a 2-D grid whose rows (2000 points) are no multiple of 512 -- stored by VIRTUAL grid lines (200 points,
    // a flat plan: csrc/grid.hip) -- on a multi-device context: the ghost range of a device is ONE row of the grid.  Bits of one device.
    const std::vector<vex::backend::command_queue> &q = ctx.queue();
    if (q.size() < 2) return;
    const size_t W = 2000, Hr = 64 * q.size(), N = W * Hr;
    std::vector<int> row(1, 0), col; std::vector<double> val;
    for (size_t k = 0, idx = 0; k < Hr; ++k) for (size_t i = 0; i < W; ++i, ++idx) {
        if (i == 0 || i == W - 1 || k == 0 || k == Hr - 1) { col.push_back((int)idx); val.push_back(1); }
        else for (long d : {-(long)W, -1l, 0l, 1l, (long)W}) { col.push_back((int)(idx + d)); val.push_back(d ? -0.25 * (d > 0 ? 3 : 1) : 4.5); }
        row.push_back((int)col.size());
    }
    const std::vector<size_t> part = vex::partition(N, q);
    for (unsigned d = 0; d < q.size(); ++d) CHECK((part[d + 1] - part[d]) % W == 0);
    setenv("VEXHIP_PLANE_FORCE", "1", 1);
    struct unforce { ~unforce() { unsetenv("VEXHIP_PLANE_FORCE"); } } unforce_at_exit;
    vex::SpMat<double, int, int> A(q, N, N, row.data(), col.data(), val.data());
    CHECK(std::string(A.step_kind()).find("one launch per device") == 0);
    if (std::string(A.step_kind()).find("one launch per device") != 0) std::cerr << "2-D: one-launch step declined: " << A.halo_declined() << std::endl;
    for (unsigned d = 0; d < q.size(); ++d) CHECK(A.storage_info(d).grid.usable == 1 && A.storage_info(d).grid.flat == 1 && A.storage_info(d).grid.nx == 200);
    std::vector<vex::backend::command_queue> q1(1, q[0]);
    vex::SpMat<double, int, int> A1(q1, N, N, row.data(), col.data(), val.data());
    std::vector<double> x = random_vector<double>(N), y1(N), ym(N);
    vex::vector<double> X(ctx, x), Y(ctx, N), X1(q1, x), Y1(q1, N);
    auto same_bits = [&]() { vex::copy(Y, ym); vex::copy(Y1, y1); for (size_t i = 0; i < N; ++i) if (std::memcmp(&ym[i], &y1[i], 8)) return false; return true; };
    Y = A * X; Y1 = A1 * X1;
    CHECK(same_bits());
    for (int rep = 0; rep < 20; ++rep) { Y = A * X; X = 0.5 * X + 0.25; Y += 1.5 * (A * X); X1 = 0.5 * X1 + 0.25; }
    Y1 = A1 * X1; Y = A * X;
    CHECK(same_bits());
    Y = X; Y += 2.5 * (A * X); Y -= A * X; Y1 = X1; Y1 += 2.5 * (A1 * X1); Y1 -= A1 * X1;
    CHECK(same_bits());
    std::vector<size_t> r2(row.begin(), row.end()), c2(col.begin(), col.end());
    vex::copy(X, x);
    auto want = host_spmv(r2, c2, val, x);
    Y = A * X; vex::copy(Y, ym);
    for (size_t i = 0; i < N; i += 53) CHECK_CLOSE(ym[i], want[i], 1e-8);
}

TEST_CASE(spmv_nonsquare_and_index_types) {                          // spmv.cpp:61-114
    const size_t n = 1024, m = 2 * n;
    std::vector<size_t> row; std::vector<int> col; std::vector<double> val;
    random_matrix(n, m, 16, row, col, val);
    std::vector<double> x = random_vector<double>(m);
    auto want = host_spmv(row, col, val, x);
    vex::SpMat<double, int> A(ctx, n, m, row.data(), col.data(), val.data());
    vex::vector<double> X(ctx, x), Y(ctx, n);
    Y = A * X;
    std::vector<double> got(n); vex::copy(Y, got);
    for (size_t i = 0; i < n; ++i) CHECK_CLOSE(got[i], want[i], 1e-8);
    std::vector<unsigned> row_u(row.begin(), row.end());
    vex::SpMat<double, int, unsigned> B(ctx, n, m, row_u.data(), col.data(), val.data());
    Y = B * X;
    vex::copy(Y, got);
    for (size_t i = 0; i < n; ++i) CHECK_CLOSE(got[i], want[i], 1e-8);
}

TEST_CASE(spmv_empty_rows) {                                         // spmv.cpp:116-146
    const size_t n = 1024, non_empty = 256;
    std::vector<size_t> row, col; std::vector<double> val;
    random_matrix(non_empty, n, 16, row, col, val);
    while (row.size() < n + 1) row.push_back(row.back());
    std::vector<double> x = random_vector<double>(n);
    auto want = host_spmv(row, col, val, x);
    vex::SpMat<double> A(ctx, n, n, row.data(), col.data(), val.data());
    vex::vector<double> X(ctx, x), Y(ctx, n);
    Y = 77; Y = A * X;                                               // empty parts zero-fill on SET
    std::vector<double> got(n); vex::copy(Y, got);
    for (size_t i = 0; i < n; ++i) CHECK_CLOSE(got[i], want[i], 1e-8);
}

static void poisson(size_t n, std::vector<size_t> &row, std::vector<unsigned> &col, std::vector<double> &val) {
    const double h2i = (n - 1) * (n - 1);                            // examples/benchmark.cpp:364-415
    row.assign(1, 0); col.clear(); val.clear();
    for (size_t k = 0, idx = 0; k < n; k++) for (size_t j = 0; j < n; j++) for (size_t i = 0; i < n; i++, idx++) {
        if (i == 0 || i == n - 1 || j == 0 || j == n - 1 || k == 0 || k == n - 1) {
            col.push_back(idx); val.push_back(1); row.push_back(row.back() + 1);
        } else {
            const long off[] = {-(long)(n * n), -(long)n, -1, 0, 1, (long)n, (long)(n * n)};
            for (int q = 0; q < 7; ++q) { col.push_back(idx + off[q]); val.push_back(q == 3 ? 6 * h2i : -h2i); }
            row.push_back(row.back() + 7);
        }
    }
}

TEST_CASE(spmv_poisson_with_ghost_planes) {                          // spmv.cpp:148-231 grid, SpMat instead of CCSR
    const size_t n = 32, N = n * n * n;
    std::vector<size_t> row; std::vector<unsigned> col; std::vector<double> val;
    poisson(n, row, col, val);
    std::vector<double> x = random_vector<double>(N);
    auto want = host_spmv(row, col, val, x);
    vex::SpMat<double, unsigned> A(ctx, N, N, row.data(), col.data(), val.data());
    vex::vector<double> X(ctx, x), Y(ctx, N);
    Y = A * X;
    std::vector<double> got(N); vex::copy(Y, got);
    double h2i = (n - 1) * (n - 1);
    for (size_t i = 0; i < N; ++i) CHECK_SMALL(got[i] - want[i], 1e-10 * 12 * h2i);
    for (int rep = 0; rep < 5; ++rep) Y += A * X;                    // repeated products reuse the exchange buffers
    vex::copy(Y, got);
    for (size_t i = 0; i < N; i += 17) CHECK_SMALL(got[i] - 6 * want[i], 1e-9 * 12 * h2i);
}

TEST_CASE(spmv_ccsr_poisson) {                                       // spmv.cpp:148-231
    const size_t n = 32, N = n * n * n;
    const double h2i = (n - 1) * (n - 1);
    std::vector<size_t> idx; idx.reserve(N);
    std::vector<size_t> row = {0, 1, 8};
    std::vector<int> col = {0, -(int)(n * n), -(int)n, -1, 0, 1, (int)n, (int)(n * n)};
    std::vector<double> val = {1, -h2i, -h2i, -h2i, 6 * h2i, -h2i, -h2i, -h2i};
    for (size_t k = 0; k < n; k++) for (size_t j = 0; j < n; j++) for (size_t i = 0; i < n; i++)
        idx.push_back((i == 0 || i == n - 1 || j == 0 || j == n - 1 || k == 0 || k == n - 1) ? 0 : 1);
    std::vector<double> x = random_vector<double>(N);
    std::vector<vex::command_queue> q1(1, ctx.queue(0));
    vex::SpMatCCSR<double, int> A(q1[0], N, 2, idx.data(), row.data(), col.data(), val.data());
    vex::vector<double> X(q1, x), Y(q1, N);
    // the same operator as an ordinary CSR matrix, checked on the host
    std::vector<size_t> prow; std::vector<unsigned> pcol; std::vector<double> pval;
    poisson(n, prow, pcol, pval);
    auto want = host_spmv(prow, pcol, pval, x);
    Y = A * X;
    std::vector<double> got(N); vex::copy(Y, got);
    for (size_t i = 0; i < N; ++i) CHECK_SMALL(got[i] - want[i], 1e-10 * 12 * h2i);
    Y = 7; Y = 2.5 * (A * X);                                        // hand-written kernel, scaled SET
    vex::copy(Y, got);
    for (size_t i = 0; i < N; ++i) CHECK_SMALL(got[i] - 2.5 * want[i], 1e-10 * 30 * h2i);
    Y -= A * X;
    vex::copy(Y, got);
    for (size_t i = 0; i < N; i += 3) CHECK_SMALL(got[i] - 1.5 * want[i], 1e-10 * 30 * h2i);
    Y = X - A * X;                                                   // a terminal like any other
    check_sample(Y, [&](size_t i, double v) { CHECK_SMALL(v - (x[i] - want[i]), 1e-9 * 12 * h2i); });
    Y = 1; Y += A * X;
    check_sample(Y, [&](size_t i, double v) { CHECK_SMALL(v - (1 + want[i]), 1e-9 * 12 * h2i); });
    vex::Reductor<double, vex::SUM> sum(q1);
    double dot = 0; for (size_t i = 0; i < N; ++i) dot += x[i] * want[i];
    CHECK_CLOSE(sum(X * (A * X)), dot, 1e-6);
}

TEST_CASE(spmv_ccsr_irregular_operators) {                          // beyond the reference's Poisson case
    std::vector<vex::command_queue> q1(1, ctx.queue(0));
    // (a) 3-D 7-point operator, odd size (ragged last block); (b), (c) 1-D operators with wide, irregular offsets
    // and three unique rows
    for (int kind = 0; kind < 3; ++kind) {
        size_t N; std::vector<size_t> idx, row; std::vector<int> col; std::vector<double> val;
        if (kind == 0) {
            const size_t n = 37; N = n * n * n;
            row = {0, 1, 8};
            col = {0, -(int)(n * n), -(int)n, -1, 0, 1, (int)n, (int)(n * n)};
            val = {1, -1.5, -2.5, -3.5, 20, -4.5, -5.5, -6.5};
            for (size_t k = 0; k < n; k++) for (size_t j = 0; j < n; j++) for (size_t i = 0; i < n; i++)
                idx.push_back((i == 0 || i == n - 1 || j == 0 || j == n - 1 || k == 0 || k == n - 1) ? 0 : 1);
        } else {
            N = 100003;
            const int far = kind == 1 ? 3000 : 40000;
            row = {0, 1, 6, 9};
            col = {0, -far, -700, -2, 0, 5, 0, 1, far};
            val = {1, 0.5, -0.25, 2, 3, -1, 7, 0.125, -0.75};
            for (size_t i = 0; i < N; ++i) idx.push_back(i < (size_t)far || i + far >= N ? 0 : (i % 5 == 0 ? 2 : 1));
        }
        vex::SpMatCCSR<double, int> A(q1[0], N, row.size() - 1, idx.data(), row.data(), col.data(), val.data());
        std::vector<double> x = random_vector<double>(N), y0 = random_vector<double>(N), want(N), a(N), b(N);
        for (size_t i = 0; i < N; ++i) {
            double s = 0;
            for (size_t j = row[idx[i]]; j < row[idx[i] + 1]; ++j) s += val[j] * x[i + col[j]];
            want[i] = s;
        }
        vex::vector<double> X(q1, x), Y(q1, N);
        Y = A * X; vex::copy(Y, b);
        vex::vector<double> Y2(q1, N);
        Y2 = 1.0 * (A * X) + 0.0 * X;                                // the same product inside a fused kernel
        vex::copy(Y2, a);
        for (size_t i = 0; i < N; i += 5) CHECK_CLOSE(a[i] + 100, b[i] + 100, 1e-10);
        for (size_t i = 0; i < N; i += 7) CHECK_CLOSE(b[i] + 100, want[i] + 100, 1e-10);
        vex::copy(y0, Y);
        Y -= 0.5 * (A * X);                                          // scaled, appended
        vex::copy(Y, b);
        for (size_t i = 0; i < N; i += 7) CHECK_CLOSE(b[i] + 100, y0[i] - 0.5 * want[i] + 100, 1e-10);
    }
}

// The operators of (b) above in the value type T: with fewer than 32768 rows the class keeps its own kernel
// (vexhip_spmv_ccsr_f64 / _f32) by default, a larger one is handed to vexhip_spmat.  Same host loop, summed in T; the
// tolerance of the double cases scaled by the type's epsilon.
template <class T>
static void check_ccsr_operator(size_t N, int far) {
    const double eps = std::numeric_limits<T>::epsilon() / std::numeric_limits<double>::epsilon();
    std::vector<vex::command_queue> q1(1, ctx.queue(0));
    std::vector<size_t> idx, row = {0, 1, 6, 9};
    std::vector<int> col = {0, -far, -700, -2, 0, 5, 0, 1, far};
    std::vector<T> val = {1, 0.5, -0.25, 2, 3, -1, 7, 0.125, -0.75};
    for (size_t i = 0; i < N; ++i) idx.push_back(i < (size_t)far || i + far >= N ? 0 : (i % 5 == 0 ? 2 : 1));
    vex::SpMatCCSR<T, int> A(q1[0], N, row.size() - 1, idx.data(), row.data(), col.data(), val.data());
    std::vector<T> x = random_vector<T>(N), y0 = random_vector<T>(N), want(N), a(N), b(N);
    for (size_t i = 0; i < N; ++i) {
        T s = 0;
        for (size_t j = row[idx[i]]; j < row[idx[i] + 1]; ++j) s += val[j] * x[i + col[j]];
        want[i] = s;
    }
    vex::vector<T> X(q1, x), Y(q1, N);
    Y = A * X; vex::copy(Y, b);
    vex::vector<T> Y2(q1, N);
    Y2 = T(1) * (A * X) + T(0) * X;                                  // the same product inside a fused kernel
    vex::copy(Y2, a);
    for (size_t i = 0; i < N; i += 5) CHECK_CLOSE(double(a[i]) + 100, double(b[i]) + 100, 1e-10 * eps);
    for (size_t i = 0; i < N; ++i) CHECK_CLOSE(double(b[i]) + 100, double(want[i]) + 100, 1e-10 * eps);
    vex::copy(y0, Y);
    Y -= T(0.5) * (A * X);                                           // scaled, appended
    vex::copy(Y, b);
    for (size_t i = 0; i < N; ++i) CHECK_CLOSE(double(b[i]) + 100, double(y0[i]) - 0.5 * double(want[i]) + 100, 1e-10 * eps);
}

TEST_CASE(spmv_ccsr_small_and_float_operators) {
    check_ccsr_operator<double>(20011, 3000);                        // N < 32768: the class's own kernel
    check_ccsr_operator<float>(20011, 3000);
    check_ccsr_operator<float>(100003, 40000);                       // float, large: handed to vexhip_spmat (f32)
}

TEST_CASE(spmv_inline_single_queue) {                                // spmv.cpp:233-260
    const size_t n = 1024;
    std::vector<vex::command_queue> queue(1, ctx.queue(0));
    std::vector<size_t> row, col; std::vector<double> val;
    random_matrix(n, n, 16, row, col, val);
    std::vector<double> x = random_vector<double>(n);
    auto want = host_spmv(row, col, val, x);
    vex::SpMat<double> A(queue, n, n, row.data(), col.data(), val.data());
    vex::vector<double> X(queue, x), Y(queue, n);
    Y = sin(vex::make_inline(A * X));
    check_sample(Y, [&](size_t i, double v) { CHECK_CLOSE(v, std::sin(want[i]), 1e-8); });
    Y = X + 2 * vex::make_inline(A * X);
    check_sample(Y, [&](size_t i, double v) { CHECK_CLOSE(v, x[i] + 2 * want[i], 1e-8); });
    // a banded matrix is stored with 1-byte diagonal codes (SELL8): same inline terminal, other decode branch
    const size_t g = 24, N = g * g * g;
    std::vector<size_t> prow; std::vector<unsigned> pcol; std::vector<double> pval;
    poisson(g, prow, pcol, pval);
    std::vector<double> px = random_vector<double>(N);
    auto pwant = host_spmv(prow, pcol, pval, px);
    vex::SpMat<double, unsigned> P(queue, N, N, prow.data(), pcol.data(), pval.data());
    vex::vector<double> PX(queue, px), PY(queue, N);
    PY = PX - vex::make_inline(P * PX);
    std::vector<double> got(N); vex::copy(PY, got);
    const double h2i = (g - 1) * (g - 1);
    for (size_t i = 0; i < N; ++i) CHECK_SMALL(got[i] - (px[i] - pwant[i]), 1e-10 * 12 * h2i);
    PY = P * PX;
    vex::copy(PY, got);
    for (size_t i = 0; i < N; ++i) CHECK_SMALL(got[i] - pwant[i], 1e-10 * 12 * h2i);
    // 64^3: 512 slices that repeat -- the matrix keeps a dictionary of the distinct ones (vexhip_spmat_info.
    // dictionary_blocks); the inline terminal and the product read the same slices through it
    {
        const size_t g2 = 64, N2 = g2 * g2 * g2;
        std::vector<size_t> row2; std::vector<unsigned> col2; std::vector<double> val2;
        poisson(g2, row2, col2, val2);
        std::vector<double> x2 = random_vector<double>(N2);
        vex::SpMat<double, unsigned> D(queue, N2, N2, row2.data(), col2.data(), val2.data());
        CHECK(D.storage_info(0).dictionary_blocks > 0 && D.storage_info(0).slice_blocks != nullptr);
        vex::vector<double> DX(queue, x2), DY(queue, N2), DZ(queue, N2);
        DY = D * DX;
        DZ = vex::make_inline(D * DX);
        std::vector<double> a(N2), b(N2); vex::copy(DY, a); vex::copy(DZ, b);
        auto want2 = host_spmv(row2, col2, val2, x2);
        const double h2 = (g2 - 1.0) * (g2 - 1.0);
        for (size_t i = 0; i < N2; ++i) {         // (the fused kernel is free to contract a*b+c: tolerance, not bits)
            CHECK_SMALL(a[i] - want2[i], 1e-10 * 12 * h2);
            CHECK_SMALL(b[i] - want2[i], 1e-10 * 12 * h2);
        }
        // the same pattern with a different value in every entry: diagonal codes + stored values; the code part of the
        // slices is pooled, the values are read where they are
        for (size_t k = 0; k < val2.size(); ++k) val2[k] *= 1.0 + 1e-6 * (double)(k % 100003);
        vex::SpMat<double, unsigned> E(queue, N2, N2, row2.data(), col2.data(), val2.data());
        CHECK(E.storage_info(0).format == VEXHIP_SPMAT_SELL8 && E.storage_info(0).dictionary_blocks > 0 && E.storage_info(0).code_pool != nullptr);
        DY = E * DX;
        DZ = vex::make_inline(E * DX);
        vex::copy(DY, a); vex::copy(DZ, b);
        auto want3 = host_spmv(row2, col2, val2, x2);
        for (size_t i = 0; i < N2; ++i) {
            CHECK_SMALL(a[i] - want3[i], 1e-10 * 13 * h2);
            CHECK_SMALL(b[i] - want3[i], 1e-10 * 13 * h2);
        }
        // round 4: the matrix stored by grid line straight from the CSR arrays (the default above 2^23 rows; forced here on the
        // 64 x 64 x 64 grid): no slices, no dictionary -- the inline terminal reads the class of the row's line and the class table
        setenv("VEXHIP_PLANE_FORCE", "1", 1);
        poisson(g2, row2, col2, val2);
        vex::SpMat<double, unsigned> G(queue, N2, N2, row2.data(), col2.data(), val2.data());
        unsetenv("VEXHIP_PLANE_FORCE");
        CHECK(G.storage_info(0).grid.usable && G.storage_info(0).grid.nx == 64 && G.storage_info(0).grid.classes == 2
              && G.storage_info(0).sell == nullptr && G.storage_info(0).code_pool == nullptr && G.storage_info(0).dictionary_blocks == 0);
        DY = G * DX;
        DZ = vex::make_inline(G * DX);
        vex::copy(DY, a); vex::copy(DZ, b);
        for (size_t i = 0; i < N2; ++i) {
            CHECK_SMALL(a[i] - want2[i], 1e-10 * 12 * h2);
            CHECK_SMALL(b[i] - want2[i], 1e-10 * 12 * h2);
        }
        DY = DX - 0.5 * (G * DX);
        vex::copy(DY, a);
        for (size_t i = 0; i < N2; i += 7) CHECK_SMALL(a[i] - (x2[i] - 0.5 * want2[i]), 1e-10 * 12 * h2);
    }
}

// Round 6: `y = z - A * x` and its relatives -- one vector, one product term -- are handed to the product whole
// (operations.hpp axpby_shape -> SpMat::apply_axpby -> vexhip_spmat_apply_axpby_f64): the plane product adds the vector in its own pass.
// The reference's two passes ("y = z", then "y -= A * x": vector.hpp:698-801) give the same bits: round(beta z) + round(alpha (A x)_i).
TEST_CASE(spmv_one_vector_one_product_single_queue) {
    std::vector<vex::command_queue> queue(1, ctx.queue(0));
    auto same_bits = [](const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; };
    // (a) 7-point operator on a 512 x 6 x 8 box: stored by grid line, 512-point lines -> the plane product
    const size_t nx = 512, ny = 6, nz = 8, N = nx * ny * nz;
    std::vector<size_t> row(1, 0); std::vector<unsigned> col; std::vector<double> val;
    for (size_t k = 0; k < nz; ++k) for (size_t j = 0; j < ny; ++j) for (size_t i = 0; i < nx; ++i) {
        const size_t r = (k * ny + j) * nx + i;
        const bool inner = i > 0 && i + 1 < nx && j > 0 && j + 1 < ny && k > 0 && k + 1 < nz;
        if (!inner) { col.push_back((unsigned)r); val.push_back(1.0); }
        else {
            const long off[7] = {-(long)(nx * ny), -(long)nx, -1, 0, 1, (long)nx, (long)(nx * ny)};
            for (int p = 0; p < 7; ++p) { col.push_back((unsigned)((long)r + off[p])); val.push_back(p == 3 ? 6.5 : -1.25); }
        }
        row.push_back(col.size());
    }
    std::vector<double> x = random_vector<double>(N), z = random_vector<double>(N);
    auto want = host_spmv(row, col, val, x);
    setenv("VEXHIP_PLANE_FORCE", "1", 1);
    vex::SpMat<double, unsigned> A(queue, N, N, row.data(), col.data(), val.data());
    unsetenv("VEXHIP_PLANE_FORCE");
    CHECK(A.storage_info(0).plane.usable && std::string(A.storage_info(0).product) == "sell8_plane_kernel");
    vex::vector<double> X(queue, x), Z(queue, z), Y(queue, N), T(queue, N);
    std::vector<double> a(N), b(N);
    Y = Z - A * X;                       T = Z; T -= A * X;
    vex::copy(Y, a); vex::copy(T, b); CHECK(same_bits(a, b));
    for (size_t i = 0; i < N; i += 3) CHECK_SMALL(a[i] - (z[i] - want[i]), 1e-12 * 20);
    Y = X + 2 * vex::make_inline(A * X); T = X; T += 2 * (A * X);
    vex::copy(Y, a); vex::copy(T, b); CHECK(same_bits(a, b));
    for (size_t i = 0; i < N; i += 3) CHECK_SMALL(a[i] - (x[i] + 2 * want[i]), 1e-12 * 40);
    Y = 3 * Z + A * X;                   T = 3 * Z; T += A * X;
    vex::copy(Y, a); vex::copy(T, b); CHECK(same_bits(a, b));
    Y = -Z - 2 * (A * X);                T = -Z; T -= 2 * (A * X);
    vex::copy(Y, a); vex::copy(T, b); CHECK(same_bits(a, b));
    Y = 0.5 * (A * X) - Z * 0.25;        T = -0.25 * Z; T += 0.5 * (A * X);
    vex::copy(Y, a); vex::copy(T, b); CHECK(same_bits(a, b));
    Y = Z; T = Z;
    Y = Y - A * X;                       T -= A * X;                     // the vector is the target itself
    vex::copy(Y, a); vex::copy(T, b); CHECK(same_bits(a, b));
    Y = X - vex::make_inline(A * X);     T = X; T -= A * X;              // the vector is x itself: taken from the registers that hold it
    vex::copy(Y, a); vex::copy(T, b); CHECK(same_bits(a, b));
    // views into larger vectors start at odd elements: the product that wants 16-byte addresses declines, the general route runs
    // (b) an unstructured matrix (32-bit columns): no product that adds a vector -- SpMat::apply_axpby declines, the general route runs
    const size_t n = 4096;
    std::vector<size_t> r2, c2; std::vector<double> v2;
    random_matrix(n, n, 16, r2, c2, v2);
    std::vector<double> x2 = random_vector<double>(n), z2 = random_vector<double>(n);
    vex::SpMat<double> R(queue, n, n, r2.data(), c2.data(), v2.data());
    vex::vector<double> X2(queue, x2), Z2(queue, z2), Y2(queue, n), T2(queue, n);
    std::vector<double> a2(n), b2(n);
    Y2 = Z2 - R * X2;                    T2 = Z2; T2 -= R * X2;
    vex::copy(Y2, a2); vex::copy(T2, b2); CHECK(same_bits(a2, b2));
    Y2 = X2 + 2 * vex::make_inline(R * X2);                             // (this product takes no addend: the terminal stays in the fused kernel, which may contract a * b + c)
    vex::copy(Y2, a2);
    auto w2 = host_spmv(r2, c2, v2, x2);
    for (size_t i = 0; i < n; ++i) CHECK_CLOSE(a2[i], x2[i] + 2 * w2[i], 1e-8);
    // float matrices: the fp32 plane product takes the addend too
    {
        std::vector<float> vf(val.begin(), val.end()), xf(x.begin(), x.end()), zf(z.begin(), z.end());
        setenv("VEXHIP_PLANE_FORCE", "1", 1);
        vex::SpMat<float, unsigned> F(queue, N, N, row.data(), col.data(), vf.data());
        unsetenv("VEXHIP_PLANE_FORCE");
        CHECK(std::string(F.storage_info(0).product) == "sell8_plane_f32_kernel");
        vex::vector<float> XF(queue, xf), ZF(queue, zf), YF(queue, N), TF(queue, N);
        std::vector<float> af(N), bf(N);
        YF = ZF - F * XF;                TF = ZF; TF -= F * XF;
        vex::copy(YF, af); vex::copy(TF, bf); CHECK(std::memcmp(af.data(), bf.data(), N * sizeof(float)) == 0);
        YF = XF + 2 * vex::make_inline(F * XF); TF = XF; TF += 2 * (F * XF);
        vex::copy(YF, af); vex::copy(TF, bf); CHECK(std::memcmp(af.data(), bf.data(), N * sizeof(float)) == 0);
    }
    // expressions of any other shape keep the general route
    Y2 = sin(Z2) - R * X2;               T2 = sin(Z2); T2 -= R * X2;
    vex::copy(Y2, a2); vex::copy(T2, b2); CHECK(same_bits(a2, b2));
}

TEST_CASE(sparse_csr_ell_matrix_single_queue) {                      // sparse_matrices.cpp:66-151
    const size_t n = 1024;
    std::vector<vex::command_queue> queue(1, ctx.queue(0));
    std::vector<int> row, col; std::vector<double> val;
    random_matrix(n, n, 16, row, col, val);
    std::vector<double> x = random_vector<double>(n);
    auto want = host_spmv(row, col, val, x);
    vex::vector<double> X(queue, x), Y(queue, n);
    {
        vex::sparse::csr<double> A(queue, n, n, row, col, val);
        Y = A * X;
        check_sample(Y, [&](size_t i, double v) { CHECK_CLOSE(v, want[i], 1e-8); });
        Y = X + A * (X * 2);                                         // x operand is an expression
        check_sample(Y, [&](size_t i, double v) { CHECK_CLOSE(v, x[i] + 2 * want[i], 1e-8); });
    }
    {
        vex::sparse::ell<double> A(queue, n, n, row, col, val);
        CHECK(A.width() > 0 && A.width() <= 15);
        Y = A * X;
        std::vector<double> got(n); vex::copy(Y, got);
        for (size_t i = 0; i < n; ++i) CHECK_CLOSE(got[i], want[i], 1e-8);
    }
    {
        vex::sparse::matrix<double> A(queue, n, n, row, col, val);
        Y = 3 * (A * X) - X;
        check_sample(Y, [&](size_t i, double v) { CHECK_CLOSE(v, 3 * want[i] - x[i], 1e-8); });
        vex::Reductor<double, vex::SUM> sum(queue);
        double s = 0; for (size_t i = 0; i < n; ++i) s += x[i] * want[i];
        CHECK_CLOSE(sum(X * (A * X)), s, 1e-8);                      // product inside a reduction
    }
}

TEST_CASE(sparse_distributed_tridiagonal_all_rows) {                 // sparse_matrices.cpp:153-193
    const size_t n = 1024;
    std::vector<int> row(1, 0), col; std::vector<double> val;
    for (size_t i = 0; i < n; ++i) {
        if (i > 0) { col.push_back(i - 1); val.push_back(-1); }
        col.push_back(i); val.push_back(2);
        if (i + 1 < n) { col.push_back(i + 1); val.push_back(-1); }
        row.push_back(col.size());
    }
    std::vector<double> x = random_vector<double>(n);
    auto want = host_spmv(row, col, val, x);
    vex::sparse::distributed<vex::sparse::ell<double>> A(ctx, n, n, row, col, val);
    vex::vector<double> X(ctx, x), Y(ctx, n);
    Y = A * X;
    std::vector<double> got(n); vex::copy(Y, got);
    for (size_t i = 0; i < n; ++i) CHECK_CLOSE(got[i], want[i], 1e-8);
    Y = X - A * X;
    vex::copy(Y, got);
    for (size_t i = 0; i < n; ++i) CHECK_SMALL(got[i] - (x[i] - want[i]), 1e-12);
    vex::sparse::distributed<vex::sparse::matrix<double>> B(ctx, n, n, row, col, val);
    Y = B * (2 * X);                                                 // expression operand on several devices
    vex::copy(Y, got);
    for (size_t i = 0; i < n; ++i) CHECK_CLOSE(got[i], 2 * want[i], 1e-8);
}

TEST_CASE(sparse_distributed_single_queue_random) {                  // sparse_matrices.cpp:195-237
    const size_t n = 1024;
    std::vector<vex::command_queue> queue(1, ctx.queue(0));
    std::vector<int> row, col; std::vector<double> val;
    random_matrix(n, n, 16, row, col, val);
    std::vector<double> x = random_vector<double>(n);
    auto want = host_spmv(row, col, val, x);
    vex::sparse::distributed<vex::sparse::csr<double>> A(queue, n, n, row, col, val);
    vex::vector<double> X(queue, x), Y(queue, n);
    Y = A * X;
    check_sample(Y, [&](size_t i, double v) { CHECK_CLOSE(v, want[i], 1e-8); });
}
