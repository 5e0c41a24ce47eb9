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
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <tuple>

#include "cf_factor_io.hpp"
#include "cf_knn_cli.hpp"
#include "cf_mf_cli.hpp"
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

    const bool from_graph = !knn.graph.empty();
    cf_ctx* ctx = nullptr;
    cfmf::Factors fu, fv;
    cfknn::Source g;
    std::vector<double> bu, bi;
    if (from_graph) {
        ctx = cfcli::open_device();
        g = cfknn::load(ctx, knn.graph, matrix);
    } else {
        fu = cfmf::read_factors(factors + ".U");
        fv = cfmf::read_factors(factors + ".V");
        if (fu.width != fv.width)
            cfcli::die("factor line of another width: " + factors + ".U holds " + std::to_string(fu.width) +
                       " values per line, " + factors + ".V " + std::to_string(fv.width));
        if (fu.width > CF_ALS_MAX_D)
            cfcli::die("D = " + std::to_string(fu.width) + " is above " + std::to_string(CF_ALS_MAX_D));
        if (bias) {
            bu = cfmf::read_bias(factors + ".bias.U", fu);
            bi = cfmf::read_bias(factors + ".bias.V", fv);
        }
    }
    const cfio::IdMap& uids = from_graph ? g.users : fu.ids;
    const cfio::IdMap& mids = from_graph ? g.items : fv.ids;
    const uint32_t D = fu.width, nu = uids.size(), nm = mids.size();

    // exclusions: the TRAIN edges as a CSR by user; held out: the VALIDATE edges by user, then item
    std::vector<uint32_t> eu, em;
    std::vector<std::tuple<uint32_t, uint32_t, float>> held;
    for (const cfio::RoleRating& r : from_graph ? g.roles : cfio::load_movielens_roles(matrix)) {
        const auto u = uids.at.find(r.user);
        if (u == uids.at.end())
            cfcli::die("user " + std::to_string(r.user) + " of " + matrix + " has no line in " + factors + ".U_*");
        const auto m = mids.at.find(r.item);
        if (m == mids.at.end())
            cfcli::die("item " + std::to_string(r.item) + " of " + matrix + " has no line in " + factors + ".V_*");
        if (r.role == cfio::kTrain) {
            eu.push_back(u->second);
            em.push_back(m->second);
        } else if (r.role == cfio::kValidate) {
            held.emplace_back(u->second, m->second, r.obs);
        }
    }
    cfmf::Csr excl = cfmf::build_csr(nu, eu, em, std::vector<float>(eu.size(), 0.0f));
    if (excl.nbr.empty()) excl.nbr.push_back(0);   // a valid pointer for an empty list
    const cfrank::Held h = cfrank::build_held(std::move(held), nu, uids, mids, matrix);
    const std::vector<uint64_t>& hoff = h.off;
    const std::vector<uint32_t>& hitem = h.item;
    const std::vector<double>& hw = h.w;

    if (from_graph) std::printf("Users: %u items: %u\n", nu, nm);
    else std::printf("Users: %u items: %u D: %u\n", nu, nm, D);
    std::vector<uint32_t> rank(hitem.size(), 0);
    std::vector<cf_rank_user> users((size_t)nu + 1);
    cf_rank_summary s{};
    if (from_graph) {
        cfcli::check(ctx,
                     cf_knn_rank_eval(ctx, nu, g.profile.off.data(), g.profile.nbr.data(), g.profile.obs.data(),
                                      knn.score_mode, knn.w_min, excl.off.data(), excl.nbr.data(), hoff.data(), hitem.data(),
                                      weighted ? hw.data() : nullptr, N, rank.data(), users.data(), &s),
                     "cf_knn_rank_eval");
    } else {
        ctx = cfcli::open_device();
        cfcli::check(ctx,
                     cf_mf_rank_eval(ctx, nu, nm, D, fu.F.data(), fv.F.data(), bias ? bu.data() : nullptr,
                                     bias ? bi.data() : nullptr, mean, excl.off.data(), excl.nbr.data(), hoff.data(),
                                     hitem.data(), weighted ? hw.data() : nullptr, N, rank.data(), users.data(), &s),
                     "cf_mf_rank_eval");
    }
    cfrank::print_rank_summary(s, h.n);
    if (!output.empty()) cfrank::write_ranks(output, nshards, uids, mids, h, rank, users);
    cf_destroy(ctx);
    return 0;
}
