// svd -- drop-in for svd.cpp: the leading singular triplets of a rating matrix by restarted
// Golub-Kahan-Lanczos on the GPU (cf_svd_fit).
//   svd.cpp:251-284  loader (cf_svd_io.hpp)
//   svd.cpp:304-505  lanczos(): the passes, "Singular value %d \t%13.6g\tError estimate: %13.6g",
//                    with --save_vectors the files <predictions>U.<i> and <predictions>V.<i>
//   svd.cpp:528-561  options; --engine, --debug and --quiet are accepted and ignored, and so is
//                    --no_edge_data, which the reference declares and never reads
//   svd.cpp:671      <predictions>singular_values: all nsv + nv + 1 + max_iter slots of sigma
// Initial vector: --initial_vector FILE, or uniform in [0, 1) from --seed (the reference: randu).
#include <cmath>
#include <cstdio>
#include <stdexcept>

#include "cf_mf_cli.hpp"
#include "cf_svd_io.hpp"

int main(int argc, char** argv) {
    const std::string dir = cfmf::matrix_dir(argc, argv);
    const auto flag = [&](const char* name) {
        const std::string v = cfcli::opt(argc, argv, name, "0");
        return v == "1" || v == "true";
    };
    const long rows_arg = std::stol(cfcli::opt(argc, argv, "rows", "-1"));
    const long cols_arg = std::stol(cfcli::opt(argc, argv, "cols", "-1"));
    const uint32_t nsv = (uint32_t)std::stoul(cfcli::opt(argc, argv, "nsv", "0"));
    const uint32_t nv = (uint32_t)std::stoul(cfcli::opt(argc, argv, "nv", "0"));
    const uint32_t max_iter = (uint32_t)std::stoul(cfcli::opt(argc, argv, "max_iter", "10"));
    const double tol = std::stod(cfcli::opt(argc, argv, "tol", "1e-8"));
    const uint32_t ortho_repeats = (uint32_t)std::stod(cfcli::opt(argc, argv, "ortho_repeats", "3"));   // a double there
    const double regularization = std::stod(cfcli::opt(argc, argv, "regularization", "0"));
    const std::string vecfile = cfcli::opt(argc, argv, "initial_vector", "");
    const std::string predictions = cfcli::opt(argc, argv, "predictions", "");
    const bool save_vectors = flag("save_vectors"), use_ids = flag("id");
    const uint64_t seed = std::stoull(cfcli::opt(argc, argv, "seed", "0"));
    const int nshards = std::stoi(cfcli::opt(argc, argv, "nshards", "4"));
    if (std::stoi(cfcli::opt(argc, argv, "unittest", "0")) != 0)
        cfcli::die("--unittest needs the gklanczos_test* directories, which were never shipped");
    if (rows_arg <= 0 || cols_arg <= 0) cfcli::die("Please specify number of rows/cols of the input matrix");
    if (nv < nsv)
        cfcli::die("Please set the number of vectors --nv=XX, to be at least the number of support vectors --nsv=XX or larger");
    if (nv > CF_SVD_MAX_NV) cfcli::die("--nv must be at most " + std::to_string(CF_SVD_MAX_NV));
    if (ortho_repeats < 1 || ortho_repeats > 3) cfcli::die("--ortho_repeats must be 1, 2 or 3");
    const uint32_t rows = (uint32_t)rows_arg, cols = (uint32_t)cols_arg;

    std::printf("Loading graph.\n");
    cfsvdio::Matrix m;
    std::vector<double> v0;
    try {
        m = cfsvdio::load_matrix(dir, vecfile, rows, cols);
        if (!vecfile.empty()) {
            std::printf("Load inital vector from file%s\n", vecfile.c_str());
            v0 = cfsvdio::load_initial_vector(vecfile, rows);
        }
    } catch (const std::exception& e) {
        cfcli::die(e.what());
    }
    if (m.row.empty()) cfcli::die("Failed to load graph. Aborting");
    if (rows == cols) cfsvdio::fold_diagonal(m, rows, regularization);   // ignored otherwise, as there
    if (v0.empty()) {
        v0.resize(rows);
        const uint64_t key = cfmf::splitmix64(seed + 0x9E3779B97F4A7C15ull);
        for (uint32_t i = 0; i < rows; ++i)
            v0[i] = (double)(cfmf::splitmix64(key ^ (uint64_t)i) >> 11) * (1.0 / 9007199254740992.0);
    }
    const cfmf::Csr by_row = cfmf::build_csr(rows, m.row, m.col, m.val);
    const cfmf::Csr by_col = cfmf::build_csr(cols, m.col, m.row, m.val);

    // sigma has the reference's data_size slots; only the first nv are ever written
    std::vector<double> sigma((size_t)nsv + nv + 1 + max_iter, 0.0), errest(std::max<uint32_t>(nv, 1), 0.0);
    std::vector<double> err(std::max<uint32_t>(nsv, 1), 0.0), U((size_t)nsv * rows), V((size_t)nsv * cols);
    cf_svd_stats st{};
    std::printf("Running SVD (gklanczos)\n");
    if (nsv) {   // nsv = 0 (the default): the reference's loop body never runs
        cf_ctx* ctx = cfcli::open_device();
        cfcli::check(ctx,
                     cf_svd_fit(ctx, rows, cols, by_row.off.data(), by_row.nbr.data(), by_row.obs.data(), by_col.off.data(),
                                by_col.nbr.data(), by_col.obs.data(), nsv, nv, max_iter, tol, ortho_repeats, v0.data(),
                                sigma.data(), errest.data(), err.data(), U.data(), V.data(), nullptr, nullptr, &st),
                     "cf_svd_fit");
        cf_destroy(ctx);
    }
    std::printf(" Number of computed signular values %u\n", st.nconv);
    const uint32_t n_out = std::min(nsv, st.nconv);
    for (uint32_t i = 0; i < n_out; ++i)
        std::printf("Singular value %d \t%13.6g\tError estimate: %13.6g\n", (int)i, sigma[i], err[i]);
    std::printf("Passes: %u  products: %u  product kernels: %.3f ms  orthogonalisation: %.3f ms  rotation: %.3f ms\n",
                st.passes, st.products, st.matvec_ms, st.ortho_ms, st.rotate_ms);
    try {
        if (save_vectors) {
            if (st.nconv == 0) cfcli::die("No converged vectors. Aborting the save operation");
            std::printf("Saving predictions to files: %s.U.* and %s.V.*\n", predictions.c_str(), predictions.c_str());
            // the reference saves nsv files per side; vectors past nconv are whatever the last pass left,
            // here only the converged ones exist
            for (uint32_t i = 0; i < n_out; ++i) {
                cfsvdio::write_vector(predictions + "U." + std::to_string(i), nshards, use_ids, 1, U.data() + (size_t)i * rows, rows);
                cfsvdio::write_vector(predictions + "V." + std::to_string(i), nshards, use_ids, rows == cols ? 0 : rows,
                                      V.data() + (size_t)i * cols, cols);
            }
        }
        cfsvdio::write_singular_values(predictions + "singular_values", sigma.data(), sigma.size());
    } catch (const std::exception& e) {
        cfcli::die(e.what());
    }
    return 0;
}
