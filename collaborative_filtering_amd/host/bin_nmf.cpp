// nmf -- non-negative matrix factorization of movielens/ ratings under the generalised
// Kullback-Leibler divergence on the GPU (cf_nmf_fit; Lee and Seung's multiplicative rules).
// Takes nmf.cpp's place among the drop-ins but not its arithmetic: nmf.cpp sums the rule's
// numerator over every edge of the graph into one vector for all vertices, so its vertices do not
// get factors of their own.  Its setRandom() start in [-1, 1] is wrong for NMF as well: a
// multiplicative rule keeps the sign of a component and a negative one makes U_u.V_i <= 0 possible.
//   loader        cf_mf_cli.hpp's: role by file suffix, "user item [rating]"; a rating outside
//                 [--minval (default 0), --maxval (default 1e100)] is fatal
//   --grid 1      (default) every user x item pair is fitted, the unrated ones as 0 (CF_NMF_GRID:
//                 implicit feedback); --grid 0 fits the rated pairs only (CF_NMF_OBSERVED)
//   --max_iter S  sweeps (default 10); one "loss" line per half-sweep
//   VALIDATE      loaded, counted and part of the RMSE line, not of the fit
//   --predictions P: P (the unclamped scores of the PREDICT pairs, as nmf.cpp's
//                 prediction_saver), P.U, P.V in als's format, which bin/recommend --factors P and
//                 bin/rankeval --factors P read unchanged
// Options: --D, --max_iter, --grid, --seed, --nshards, --predictions, --minval, --maxval.
// Initial factors: max(0.5 (x + 1), CF_NMF_EPS) of cf_mf_cli.hpp's draw x, uniform in [0, 1).
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "cf_mf_cli.hpp"

int main(int argc, char** argv) {
    const std::string dir = cfmf::matrix_dir(argc, argv);
    const uint32_t D = (uint32_t)std::stoul(cfcli::opt(argc, argv, "D", "20"));
    const uint32_t sweeps = (uint32_t)std::stoul(cfcli::opt(argc, argv, "max_iter", "10"));
    const int grid = std::stoi(cfcli::opt(argc, argv, "grid", "1"));
    const double minval = std::stod(cfcli::opt(argc, argv, "minval", "0"));
    const double maxval = std::stod(cfcli::opt(argc, argv, "maxval", "1e100"));
    const std::string predictions = cfcli::opt(argc, argv, "predictions", "");
    const uint64_t seed = std::stoull(cfcli::opt(argc, argv, "seed", "0"));
    const int nshards = std::stoi(cfcli::opt(argc, argv, "nshards", "4"));
    if (D == 0 || D > CF_ALS_MAX_D) cfcli::die("--D must be between 1 and " + std::to_string(CF_ALS_MAX_D));
    if (grid != 0 && grid != 1) cfcli::die("--grid must be 0 or 1");
    if (!(minval >= 0.0)) cfcli::die("--minval must not be negative (the divergence needs ratings >= 0)");

    const cfmf::Data data = cfmf::load(dir, minval, maxval);
    const uint32_t nu = data.nu, nm = data.nm;
    std::vector<double> U, V, trace(2 * (size_t)sweeps, 0.0);
    cfmf::init_factors(U, nu, D, seed, 0);
    cfmf::init_factors(V, nm, D, seed, 1);
    for (std::vector<double>* F : {&U, &V})
        for (double& x : *F) x = std::max(0.5 * (x + 1.0), CF_NMF_EPS);

    cf_ctx* ctx = cfcli::open_device();
    std::printf("Running NMF (%s)\n", grid ? "whole grid" : "observed pairs");
    cf_nmf_stats st{};
    const cfmf::Csr &bu = data.by_user, &bi = data.by_item;
    cfcli::check(ctx,
                 cf_nmf_fit(ctx, nu, nm, D, bu.off.data(), bu.nbr.data(), bu.obs.data(), bi.off.data(), bi.nbr.data(),
                            bi.obs.data(), grid ? CF_NMF_GRID : CF_NMF_OBSERVED, sweeps, U.data(), V.data(), trace.data(),
                            &st),
                 "cf_nmf_fit");
    for (size_t h = 0; h < trace.size(); ++h)
        std::printf("loss after sweep %zu %s half-sweep: %.17g\n", h / 2 + 1, h % 2 ? "item" : "user", trace[h]);
    double sq[2] = {0.0, 0.0};
    for (int role = 0; role < 2; ++role)
        cfcli::check(ctx,
                     cf_sgd_error(ctx, data.eu[role].size(), data.eu[role].data(), data.em[role].data(),
                                  data.eo[role].data(), nu, nm, D, U.data(), V.data(), nullptr, nullptr, 0.0, minval, maxval,
                                  &sq[role]),
                     "cf_sgd_error");
    std::printf("%s\n", cfmf::rmse_line(data, sq).c_str());
    std::printf("----------------------------------------------------------\n");
    std::printf("Sweeps: %u  column sums: %.3f ms  update kernels: %.3f ms  loss kernels: %.3f ms  floored: %llu\n", st.sweeps,
                st.sum_ms, st.update_ms, st.loss_ms, (unsigned long long)st.n_floored);
    if (st.n_floored)
        std::printf("warning: %llu components were set to the floor %g\n", (unsigned long long)st.n_floored, CF_NMF_EPS);

    if (!predictions.empty()) {
        std::printf("Saving predictions\n");
        const size_t np = data.eu[cfio::kPredict].size();
        std::vector<double> pred(np);
        cfcli::check(ctx,
                     cf_als_predict(ctx, np, data.eu[cfio::kPredict].data(), data.em[cfio::kPredict].data(), nu, nm, D,
                                    U.data(), V.data(), pred.data()),
                     "cf_als_predict");
        cfmf::write_predictions(data, predictions, nshards, pred);
        cfmf::write_vertex_values(data.uids, predictions + ".U", nshards, U, D, " ", true);
        cfmf::write_vertex_values(data.mids, predictions + ".V", nshards, V, D, ") ", true);
    }
    cf_destroy(ctx);
    return 0;
}
