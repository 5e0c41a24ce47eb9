// recommend -- the N best unrated items of every user from the factor files of als, sgd, biassgd,
// svdpp or svd (--predictions P there).  No reference counterpart: its programs save the PREDICT
// edges only (als.cpp:493-510), so scoring every item of every user meant listing every pair.
//   recommend --factors P [--matrix DIR] --topn N [--bias] [--mean M] --output R [--nshards 4] [--users FILE]
//   recommend --graph G --matrix DIR --topn N [--wmin W] [--score sum|mean] --output R [--nshards 4] [--users FILE]
//   P.U_* / P.V_*        factor lines "id f0 f1 .. " or "id) f0 f1 .. " (cf_factor_io.hpp); D is the
//                        first line's width; --bias also reads P.bias.U_* / P.bias.V_* and adds
//                        bias_item + (M + bias_user) to every score (biassgd.cpp:400-403)
//   --matrix DIR         every TRAIN and VALIDATE edge of DIR is excluded (.predict pairs stay
//                        candidates); a user or item of DIR without a factor line is fatal
//   --graph G            instead of --factors: the item graph G* (the out_fin_ shards of knn2) scores
//                        every item for a user from the user's TRAIN edges of DIR, by cf_knn_topn
//                        (cf_knn_cli.hpp): --score sum = sum of w r over the rated items with w > W
//                        (default 0.1), mean = that over the sum of those w (knn3's prediction);
//                        users are those of DIR, items those of G* and DIR together
//   --users FILE         one user id per line: only their lists, in that order (default: every
//                        user of P.U_*, ascending id)
//   R_<i>_of_<nshards>   "user\titem\tscore" per listed item in rank order per user, score as %g,
//                        sharded by user id like the predictions (cf_mf_cli.hpp write_predictions)
#include <cstdio>
#include <cstring>

#include "cf_factor_io.hpp"
#include "cf_knn_cli.hpp"
#include "cf_mf_cli.hpp"
#include "cf_rank_cli.hpp"

int main(int argc, char** argv) {
    const std::string factors = cfcli::opt(argc, argv, "factors", "");
    const std::string matrix = cfcli::opt(argc, argv, "matrix", "");
    const std::string output = cfcli::opt(argc, argv, "output", "");
    const std::string topn = cfcli::opt(argc, argv, "topn", "");
    const std::string users_file = cfcli::opt(argc, argv, "users", "");
    const double mean = std::stod(cfcli::opt(argc, argv, "mean", "0"));
    const int nshards = std::stoi(cfcli::opt(argc, argv, "nshards", "4"));
    bool bias = false;
    for (int i = 1; i < argc; ++i) bias = bias || std::strcmp(argv[i], "--bias") == 0;
    const char* usage =
        "usage: recommend --factors P [--matrix DIR] --topn N [--bias] [--mean M] --output R [--nshards 4] [--users FILE]\n"
        "       recommend --graph G --matrix DIR --topn N [--wmin W] [--score sum|mean] --output R [--nshards 4] [--users FILE]";
    if (output.empty() || topn.empty()) cfcli::die(usage);
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
    const std::string ufile = from_graph ? matrix : factors + ".U_*";   // where a user id comes from
    const uint32_t D = fu.width, nu = uids.size(), nm = mids.size();

    // exclusions: the TRAIN and VALIDATE edges, as a CSR by user
    cfmf::Csr excl;
    if (!matrix.empty()) {
        std::vector<uint32_t> eu, em;
        for (const cfio::RoleRating& r : from_graph ? g.roles : cfio::load_movielens_roles(matrix)) {
            const auto u = uids.at.find(r.user);
            if (u == uids.at.end())
                cfcli::die("user " + std::to_string(r.user) + " of " + matrix + " has no line in " + factors + ".U_*");
            const auto m = mids.at.find(r.item);
            if (m == mids.at.end())
                cfcli::die("item " + std::to_string(r.item) + " of " + matrix + " has no line in " + factors + ".V_*");
            if (r.role == cfio::kPredict) continue;
            eu.push_back(u->second);
            em.push_back(m->second);
        }
        excl = cfmf::build_csr(nu, eu, em, std::vector<float>(eu.size(), 0.0f));
        if (excl.nbr.empty()) excl.nbr.push_back(0);   // a valid pointer for an empty list
    }

    std::vector<uint32_t> sel;
    if (!users_file.empty()) sel = cfrank::read_users(users_file, uids, ufile);
    const bool selected = !users_file.empty();
    const uint32_t n_out = selected ? (uint32_t)sel.size() : nu;
    if (selected && sel.empty()) sel.push_back(0);

    if (from_graph) std::printf("Users: %u items: %u\n", nu, nm);
    else std::printf("Users: %u items: %u D: %u\n", nu, nm, D);
    std::vector<uint32_t> items((size_t)n_out * N), count(n_out);
    std::vector<double> scores((size_t)n_out * N);
    cf_topn_stats st{};
    if (from_graph) {
        cfcli::check(ctx,
                     cf_knn_topn(ctx, nu, g.profile.off.data(), g.profile.nbr.data(), g.profile.obs.data(), knn.score_mode,
                                 knn.w_min, excl.off.data(), excl.nbr.data(), selected ? n_out : 0,
                                 selected ? sel.data() : nullptr, N, items.data(), scores.data(), count.data(), &st),
                     "cf_knn_topn");
    } else {
        ctx = cfcli::open_device();
        cfcli::check(ctx,
                     cf_mf_topn(ctx, nu, nm, D, fu.F.data(), fv.F.data(), bias ? bu.data() : nullptr,
                                bias ? bi.data() : nullptr, mean, matrix.empty() ? nullptr : excl.off.data(),
                                matrix.empty() ? nullptr : excl.nbr.data(), selected ? n_out : 0,
                                selected ? sel.data() : nullptr, N, items.data(), scores.data(), count.data(), &st),
                     "cf_mf_topn");
    }
    cfrank::print_topn_stats(st);
    cfrank::write_lists(output, nshards, uids, mids, selected, sel, n_out, N, items, scores, count);
    cf_destroy(ctx);
    return 0;
}
