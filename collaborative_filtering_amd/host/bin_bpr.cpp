// bpr -- Bayesian Personalized Ranking on the TRAIN edges of a movielens/ directory on the GPU
// (cf_bpr_fit; Rendle et al., UAI 2009).  No reference counterpart: the toolkit's other models
// fit ratings, this one the order of a user's rated items above its unrated ones, which is what
// bin/rankeval measures.
//   loader        cf_mf_cli.hpp's: role by file suffix, "user item [rating]"
//   positives     every TRAIN pair; repeated pairs are merged and the lists sorted before the call.
//                 --minrating R drops the pairs rated below R first (a dropped pair counts as unrated)
//   --bias 1      (default) item biases b_i in the score U_u.V_i + b_i; --bias 0 fits none
//   --max_iter S  sweeps (default 10), one sampled negative per positive and sweep; one "loss" line
//                 per sweep: the mean of softplus(-x) over the sweep's triples, from the factors at
//                 the start of the sweep, the triples and the skipped positives
//   VALIDATE      loaded and counted, not part of the fit (rankeval ranks them)
//   --predictions P: P (the scores of the PREDICT pairs), P.U, P.V in biassgd's format, P.bias.U
//                 (all zeros) and P.bias.V, which bin/recommend --factors P --bias and bin/rankeval
//                 --factors P --bias read unchanged with --mean 0
// Options: --D, --max_iter, --lr, --reg (all three weights), --bias, --seed, --minrating, --nshards,
// --predictions.  Initial factors: 0.1 x of cf_mf_cli.hpp's draw x, uniform in [-0.1, 0.1); biases 0.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <utility>

#include "cf_mf_cli.hpp"

int main(int argc, char** argv) {
    const std::string dir = cfmf::matrix_dir(argc, argv);
    const uint32_t D = (uint32_t)std::stoul(cfcli::opt(argc, argv, "D", "20"));
    cf_bpr_params par{};
    par.n_sweeps = (uint32_t)std::stoul(cfcli::opt(argc, argv, "max_iter", "10"));
    par.lr = std::stod(cfcli::opt(argc, argv, "lr", "0.5"));
    par.reg_user = par.reg_item = par.reg_bias = std::stod(cfcli::opt(argc, argv, "reg", "0.01"));
    par.seed = std::stoull(cfcli::opt(argc, argv, "seed", "0"));
    const int bias = std::stoi(cfcli::opt(argc, argv, "bias", "1"));
    const std::string minrating = cfcli::opt(argc, argv, "minrating", "");
    const std::string predictions = cfcli::opt(argc, argv, "predictions", "");
    const int nshards = std::stoi(cfcli::opt(argc, argv, "nshards", "4"));
    if (D == 0 || D > CF_ALS_MAX_D) cfcli::die("--D must be between 1 and " + std::to_string(CF_ALS_MAX_D));
    if (bias != 0 && bias != 1) cfcli::die("--bias must be 0 or 1");
    if (!std::isfinite(par.lr)) cfcli::die("--lr must be finite");
    if (!(par.reg_user >= 0.0) || !std::isfinite(par.reg_user)) cfcli::die("--reg must be finite and not negative");

    const cfmf::Data data = cfmf::load(dir, -1e100, 1e100);
    const uint32_t nu = data.nu, nm = data.nm;
    // the positives: the TRAIN pairs at or above --minrating, sorted by (user, item), each once
    std::vector<std::pair<uint32_t, uint32_t>> pos;
    const double floor_rating = minrating.empty() ? 0.0 : std::stod(minrating);
    for (size_t e = 0; e < data.eu[cfio::kTrain].size(); ++e)
        if (minrating.empty() || (double)data.eo[cfio::kTrain][e] >= floor_rating)
            pos.emplace_back(data.eu[cfio::kTrain][e], data.em[cfio::kTrain][e]);
    std::sort(pos.begin(), pos.end());
    pos.erase(std::unique(pos.begin(), pos.end()), pos.end());
    std::vector<uint32_t> pu(pos.size()), pm(pos.size());
    for (size_t e = 0; e < pos.size(); ++e) {
        pu[e] = pos[e].first;
        pm[e] = pos[e].second;
    }
    const std::vector<float> none(pos.size(), 0.0f);
    const cfmf::Csr by_user = cfmf::build_csr(nu, pu, pm, none), by_item = cfmf::build_csr(nm, pm, pu, none);   // stable: both ascend
    std::printf("Positive pairs: %zu\n", pos.size());

    std::vector<double> U, V, bu(nu, 0.0), bi(nm, 0.0), trace(2 * (size_t)par.n_sweeps, 0.0);
    cfmf::init_factors(U, nu, D, par.seed, 0);
    cfmf::init_factors(V, nm, D, par.seed, 1);
    for (std::vector<double>* F : {&U, &V})
        for (double& x : *F) x *= 0.1;

    cf_ctx* ctx = cfcli::open_device();
    std::printf("Running BPR (%s)\n", bias ? "item biases" : "no bias");
    cf_bpr_stats st{};
    cfcli::check(ctx,
                 cf_bpr_fit(ctx, nu, nm, D, by_user.off.data(), by_user.nbr.data(), by_item.off.data(), by_item.nbr.data(),
                            &par, U.data(), V.data(), bias ? bi.data() : nullptr, trace.data(), &st),
                 "cf_bpr_fit");
    for (uint32_t s = 0; s < st.sweeps; ++s) {
        const double triples = trace[2 * (size_t)s + 1];
        std::printf("loss at sweep %u: %.17g triples: %.0f skipped: %.0f\n", s + 1, triples > 0.0 ? trace[2 * (size_t)s] / triples : 0.0,
                    triples, (double)pos.size() - triples);
    }
    if (st.n_nan) cfcli::die("Got into numeric errors.. try to tune the step size and regularization using --lr and --reg");
    std::printf("----------------------------------------------------------\n");
    std::printf("Sweeps: %u  triples: %llu  skipped: %llu  sample kernels: %.3f ms  reduction kernels: %.3f ms  commit kernels: %.3f ms\n",
                st.sweeps, (unsigned long long)st.triples, (unsigned long long)st.n_skipped, st.sample_ms, st.reduce_ms,
                st.apply_ms);

    if (!predictions.empty()) {
        std::printf("Saving predictions\n");
        const size_t np = data.eu[cfio::kPredict].size();
        std::vector<double> pred(np);
        cfcli::check(ctx,
                     cf_sgd_predict(ctx, np, data.eu[cfio::kPredict].data(), data.em[cfio::kPredict].data(), nu, nm, D,
                                    U.data(), V.data(), bu.data(), bi.data(), 0.0, 0, 0.0, 0.0, pred.data()),
                     "cf_sgd_predict");
        cfmf::write_predictions(data, predictions, nshards, pred);
        cfmf::write_vertex_values(data.uids, predictions + ".U", nshards, U, D, " ", true);
        cfmf::write_vertex_values(data.mids, predictions + ".V", nshards, V, D, " ", true);
        cfmf::write_vertex_values(data.uids, predictions + ".bias.U", nshards, bu, 1, " ", false);
        cfmf::write_vertex_values(data.mids, predictions + ".bias.V", nshards, bi, 1, " ", false);
    }
    cf_destroy(ctx);
    return 0;
}
