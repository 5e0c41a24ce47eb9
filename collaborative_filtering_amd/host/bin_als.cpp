// als -- drop-in for als.cpp: ALS matrix factorization of movielens/ ratings on the GPU.
//   als.cpp:379-417  loader: role by file suffix (TRAIN, .validate, .predict), "user item [rating]",
//                    ratings outside [minval, maxval] are fatal for TRAIN and VALIDATE
//   als.cpp:290-371  vertex program on the synchronous engine (cf_als_fit)
//   als.cpp:424-483  error aggregate: RMSE per role of the clamped predictions (cf_als_error)
//   als.cpp:493-553  --predictions P: P (PREDICT edges), P.U (vertices with out-edges), P.V (the rest)
//   als.cpp:579-600  options
// Initial factors: cf_mf_cli.hpp (reproducible, not the reference's rand() stream).
#include <cmath>
#include <cstdio>
#include <limits>

#include "cf_mf_cli.hpp"

int main(int argc, char** argv) {
    const std::string dir = cfmf::matrix_dir(argc, argv);
    const uint32_t D = (uint32_t)std::stoul(cfcli::opt(argc, argv, "D", "20"));
    const std::string max_iter = cfcli::opt(argc, argv, "max_iter", "");
    const uint64_t max_updates = max_iter.empty() ? std::numeric_limits<uint64_t>::max() : std::stoull(max_iter);
    const double lambda = std::stod(cfcli::opt(argc, argv, "lambda", "0.01"));
    const double tol = std::stod(cfcli::opt(argc, argv, "tol", "1e-3"));
    const double maxval = std::stod(cfcli::opt(argc, argv, "maxval", "1e+100"));
    const double minval = std::stod(cfcli::opt(argc, argv, "minval", "-1e+100"));
    const int regnormal = std::stoi(cfcli::opt(argc, argv, "regnormal", "1"));
    const std::string predictions = cfcli::opt(argc, argv, "predictions", "");
    const uint64_t seed = std::stoull(cfcli::opt(argc, argv, "seed", "0"));
    const int nshards = std::stoi(cfcli::opt(argc, argv, "nshards", "4"));
    const uint32_t max_supersteps = (uint32_t)std::stoul(cfcli::opt(argc, argv, "max_supersteps", "0"));
    // --engine and --interval are accepted and ignored (one engine, one final report)
    if (std::stoi(cfcli::opt(argc, argv, "implicitratingtype", "0")) != 0)
        cfcli::die("--implicitratingtype other than 0 (implicit.hpp's added edges) is not supported");
    if (D == 0 || D > CF_ALS_MAX_D) cfcli::die("--D must be between 1 and " + std::to_string(CF_ALS_MAX_D));

    const cfmf::Data data = cfmf::load(dir, minval, maxval);
    const uint32_t nu = data.nu, nm = data.nm;
    const auto& eu = data.eu;
    const auto& em = data.em;
    const auto& eo = data.eo;
    const std::vector<double>& out_degree = data.out_degree;
    const cfmf::Csr& by_user = data.by_user;
    const cfmf::Csr& by_item = data.by_item;
    // regularisation (als.cpp:323-327): lambda, or lambda * num_out_edges -- 0 for every item
    std::vector<double> reg_u(nu, lambda), reg_m(nm, regnormal ? 0.0 : lambda);
    if (regnormal)
        for (uint32_t u = 0; u < nu; ++u) reg_u[u] = lambda * out_degree[u];
    std::vector<double> U, V;
    cfmf::init_factors(U, nu, D, seed, 0);
    cfmf::init_factors(V, nm, D, seed, 1);
    std::vector<uint32_t> nup_u(nu, 0), nup_m(nm, 0);
    std::vector<float> res_u(nu, 0.0f), res_m(nm, 0.0f);

    cf_ctx* ctx = cfcli::open_device();
    std::printf("Running ALS\n");
    cf_als_stats st{};
    // every user has an out-edge (it would not be a vertex otherwise): all are signalled (als.cpp:363-367)
    cfcli::check(ctx,
                 cf_als_fit(ctx, nu, nm, D, by_user.off.data(), by_user.nbr.data(), by_user.obs.data(), by_item.off.data(),
                            by_item.nbr.data(), by_item.obs.data(), reg_u.data(), reg_m.data(), tol, max_updates,
                            max_supersteps, U.data(), V.data(), nup_u.data(), nup_m.data(), res_u.data(), res_m.data(),
                            nullptr, &st),
                 "cf_als_fit");
    std::printf("----------------------------------------------------------\n");
    std::printf("Supersteps: %u  update kernels: %.3f ms  scatter kernels: %.3f ms\n", st.supersteps, st.update_ms,
                st.scatter_ms);
    std::printf("Updates executed: %llu\n", (unsigned long long)st.updates);
    if (st.n_not_pd)
        std::printf("warning: %llu pivots were not positive (systems outside the parity claim)\n",
                    (unsigned long long)st.n_not_pd);
    std::printf("Final error: \n");
    double sq[2] = {0.0, 0.0};
    for (int role = 0; role < 2; ++role)
        cfcli::check(ctx,
                     cf_als_error(ctx, eu[role].size(), eu[role].data(), em[role].data(), eo[role].data(), nu, nm, D,
                                  U.data(), V.data(), minval, maxval, &sq[role]),
                     "cf_als_error");
    std::printf("%s\n", cfmf::rmse_line(data, sq).c_str());

    if (!predictions.empty()) {
        std::printf("Saving predictions\n");
        const size_t np = eu[cfio::kPredict].size();
        std::vector<double> pred(np);
        cfcli::check(ctx,
                     cf_als_predict(ctx, np, eu[cfio::kPredict].data(), em[cfio::kPredict].data(), nu, nm, D, U.data(),
                                    V.data(), pred.data()),
                     "cf_als_predict");
        cfmf::write_predictions(data, predictions, nshards, pred);   // als.cpp:504-506
        cfmf::write_vertex_values(data.uids, predictions + ".U", nshards, U, D, " ", true);    // als.cpp:521-525
        cfmf::write_vertex_values(data.mids, predictions + ".V", nshards, V, D, ") ", true);   // als.cpp:542-546
    }
    cf_destroy(ctx);
    return 0;
}
