// ials -- implicit-feedback ALS (Hu, Koren, Volinsky, ICDM 2008) of movielens/ ratings on the GPU.
// No reference counterpart: wals.cpp cites the paper and fits the observed (and sampled) edges
// only; here every user x item pair is a training example (cf_ials_fit).
//   loader        cf_mf_cli.hpp's: role by file suffix, "user item [rating]"; a rating < 0 is fatal
//   TRAIN edge    preference 1 if rating > --threshold (default 0), else 0;
//                 confidence 1 + --alpha * rating (default 40, the paper's value)
//   VALIDATE      loaded and counted, not part of the fit
//   --max_iter S  sweeps (default 10); one "loss" line per half-sweep
//   --predictions P: P (the unclamped scores of the PREDICT pairs), P.U, P.V in als's format,
//                 which bin/recommend --factors P reads unchanged
// Options: --D, --lambda (added to every diagonal, default 0.1), --alpha, --threshold, --max_iter,
// --seed, --nshards, --predictions.  Initial factors: cf_mf_cli.hpp.
#include <cmath>
#include <cstdio>
#include <limits>

#include "cf_mf_cli.hpp"

int main(int argc, char** argv) {
    const std::string dir = cfmf::matrix_dir(argc, argv);
    const uint32_t D = (uint32_t)std::stoul(cfcli::opt(argc, argv, "D", "20"));
    const uint32_t sweeps = (uint32_t)std::stoul(cfcli::opt(argc, argv, "max_iter", "10"));
    const double lambda = std::stod(cfcli::opt(argc, argv, "lambda", "0.1"));
    const double alpha = std::stod(cfcli::opt(argc, argv, "alpha", "40"));
    const double threshold = std::stod(cfcli::opt(argc, argv, "threshold", "0"));
    const std::string predictions = cfcli::opt(argc, argv, "predictions", "");
    const uint64_t seed = std::stoull(cfcli::opt(argc, argv, "seed", "0"));
    const int nshards = std::stoi(cfcli::opt(argc, argv, "nshards", "4"));
    if (D == 0 || D > CF_ALS_MAX_D) cfcli::die("--D must be between 1 and " + std::to_string(CF_ALS_MAX_D));
    if (!(lambda > 0.0)) cfcli::die("--lambda must be positive (it keeps every system positive definite)");
    if (!(alpha >= 0.0)) cfcli::die("--alpha must not be negative (confidences are 1 + alpha * rating >= 1)");

    // a negative rating would give a confidence below 1: fatal, with the loader's message
    const cfmf::Data data = cfmf::load(dir, 0.0, std::numeric_limits<double>::infinity());
    const uint32_t nu = data.nu, nm = data.nm;
    // confidence and preference per TRAIN edge, in the order of each CSR
    cfmf::Csr by[2] = {data.by_user, data.by_item};
    std::vector<float> pref[2];
    for (int k = 0; k < 2; ++k) {
        pref[k].resize(by[k].obs.size());
        for (size_t e = 0; e < by[k].obs.size(); ++e) {
            const double r = (double)by[k].obs[e];
            pref[k][e] = r > threshold ? 1.0f : 0.0f;
            by[k].obs[e] = (float)(1.0 + alpha * r);
        }
    }
    std::vector<double> reg_u(nu, lambda), reg_m(nm, lambda), U, V, trace(2 * (size_t)sweeps, 0.0);
    cfmf::init_factors(U, nu, D, seed, 0);
    cfmf::init_factors(V, nm, D, seed, 1);

    cf_ctx* ctx = cfcli::open_device();
    std::printf("Running implicit-feedback ALS\n");
    cf_ials_stats st{};
    cfcli::check(ctx,
                 cf_ials_fit(ctx, nu, nm, D, by[0].off.data(), by[0].nbr.data(), by[0].obs.data(), pref[0].data(),
                             by[1].off.data(), by[1].nbr.data(), by[1].obs.data(), pref[1].data(), reg_u.data(),
                             reg_m.data(), sweeps, U.data(), V.data(), trace.data(), &st),
                 "cf_ials_fit");
    for (size_t h = 0; h < trace.size(); ++h)
        std::printf("loss after sweep %zu %s half-sweep: %.17g\n", h / 2 + 1, h % 2 ? "item" : "user", trace[h]);
    std::printf("----------------------------------------------------------\n");
    std::printf("Sweeps: %u  Gram kernels: %.3f ms  update kernels: %.3f ms  loss kernels: %.3f ms\n", st.sweeps, st.gram_ms,
                st.update_ms, st.loss_ms);
    if (st.n_not_pd)
        std::printf("warning: %llu pivots were not positive\n", (unsigned long long)st.n_not_pd);

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
