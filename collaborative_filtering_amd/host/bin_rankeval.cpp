// rankeval -- how well the factor files of als, ials, sgd, biassgd, svdpp or svd rank held-out
// edges: the exact rank of every VALIDATE edge among its user's candidate items, and precision,
// recall, NDCG, MAP, MRR, AUC and the expected percentile rank (Hu, Koren, Volinsky) at a cutoff.
// No reference counterpart: its programs report RMSE over listed pairs only.
//   rankeval --factors P --matrix DIR --topn N [--bias] [--mean M] [--weighted] [--output R] [--nshards 4]
//   rankeval --graph G --matrix DIR --topn N [--wmin W] [--score sum|mean] [--weighted] [--output R] [--nshards 4]
//   P.U_* / P.V_*        factor lines as for recommend (cf_factor_io.hpp); --bias also reads
//                        P.bias.U_* / P.bias.V_* and adds bias_item + (M + bias_user) to every score
//   --graph G            instead of --factors: the scores of recommend --graph (cf_knn_rank_eval): the
//                        item graph G* and, as the users' profiles, the TRAIN edges of DIR
//   --matrix DIR         the TRAIN edges of DIR are excluded, its VALIDATE edges are held out (their
//                        value is the edge's weight in mpr under --weighted), its PREDICT edges are
//                        ignored; a user or item of DIR without a factor line is fatal, and so is a
//                        VALIDATE pair listed twice
//   R_<i>_of_<nshards>   "user\titem\trank\tn_cand" per held-out edge, by user then item, sharded by
//                        user id like the predictions; ranks are 0-based, a skipped edge (excluded, or
//                        a NaN score) has rank -1
#include <cstdio>
#include <cstring>

#include "cf_rank_cli.hpp"

int main(int argc, char** argv) {
    const std::string factors = cfcli::opt(argc, argv, "factors", "");
    const std::string matrix = cfcli::opt(argc, argv, "matrix", "");
    const std::string output = cfcli::opt(argc, argv, "output", "");
    const std::string topn = cfcli::opt(argc, argv, "topn", "");
    const double mean = std::stod(cfcli::opt(argc, argv, "mean", "0"));
    const int nshards = std::stoi(cfcli::opt(argc, argv, "nshards", "4"));
    bool bias = false, weighted = false;
    for (int i = 1; i < argc; ++i) {
        bias = bias || std::strcmp(argv[i], "--bias") == 0;
        weighted = weighted || std::strcmp(argv[i], "--weighted") == 0;
    }
    const char* usage =
        "usage: rankeval --factors P --matrix DIR --topn N [--bias] [--mean M] [--weighted] [--output R] [--nshards 4]\n"
        "       rankeval --graph G --matrix DIR --topn N [--wmin W] [--score sum|mean] [--weighted] [--output R] [--nshards 4]";
    if (matrix.empty() || topn.empty()) cfcli::die(usage);
    const cfknn::Options knn = cfknn::options(argc, argv, factors, matrix, usage);
    const uint32_t N = (uint32_t)std::stoul(topn);
    if (N == 0 || N > CF_TOPN_MAX_N) cfcli::die("--topn must be between 1 and " + std::to_string(CF_TOPN_MAX_N));
    if (nshards < 1) cfcli::die("--nshards must be at least 1");

    cfrank::Source src;
    cfrank::load_source(src, knn, factors, matrix, bias);
    const cfio::IdMap &uids = src.uids(), &mids = src.mids();
    const uint32_t nu = uids.size(), nm = mids.size();

    // exclusions: the TRAIN edges; held out: the VALIDATE edges by user, then item
    std::vector<std::tuple<uint32_t, uint32_t, float>> held;
    const cfmf::Csr excl = cfrank::role_exclusions(src, matrix, factors, 1u << cfio::kTrain, &held);
    const cfrank::Held h = cfrank::build_held(std::move(held), nu, uids, mids, matrix);

    src.print_sizes();
    std::vector<uint32_t> rank(h.item.size(), 0);
    std::vector<cf_rank_user> users((size_t)nu + 1);
    cf_rank_summary s{};
    if (src.from_graph) {
        const cfmf::Csr& prof = src.g.profile;
        cfcli::check(src.ctx,
                     cf_knn_rank_eval(src.ctx, nu, prof.off.data(), prof.nbr.data(), prof.obs.data(), knn.score_mode,
                                      knn.w_min, excl.off.data(), excl.nbr.data(), h.off.data(), h.item.data(),
                                      weighted ? h.w.data() : nullptr, N, rank.data(), users.data(), &s),
                     "cf_knn_rank_eval");
    } else {
        src.ctx = cfcli::open_device();
        cfcli::check(src.ctx,
                     cf_mf_rank_eval(src.ctx, nu, nm, src.fu.width, src.fu.F.data(), src.fv.F.data(),
                                     bias ? src.bu.data() : nullptr, bias ? src.bi.data() : nullptr, mean, excl.off.data(),
                                     excl.nbr.data(), h.off.data(), h.item.data(), weighted ? h.w.data() : nullptr, N,
                                     rank.data(), users.data(), &s),
                     "cf_mf_rank_eval");
    }
    cfrank::print_rank_summary(s, h.n);
    if (!output.empty()) cfrank::write_ranks(output, nshards, uids, mids, h, rank, users);
    cf_destroy(src.ctx);
    return 0;
}
