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

    cfrank::Source src;
    cfrank::load_source(src, knn, factors, matrix, bias);
    const cfio::IdMap &uids = src.uids(), &mids = src.mids();
    const uint32_t nu = uids.size(), nm = mids.size();

    // exclusions: the TRAIN and VALIDATE edges
    cfmf::Csr excl;
    if (!matrix.empty())
        excl = cfrank::role_exclusions(src, matrix, factors, 1u << cfio::kTrain | 1u << cfio::kValidate, nullptr);
    // where a user id comes from
    cfrank::Lists l = cfrank::make_lists(users_file, uids, src.from_graph ? matrix : factors + ".U_*", nu, N);

    src.print_sizes();
    cf_topn_stats st{};
    if (src.from_graph) {
        const cfmf::Csr& prof = src.g.profile;
        cfcli::check(src.ctx,
                     cf_knn_topn(src.ctx, nu, prof.off.data(), prof.nbr.data(), prof.obs.data(), knn.score_mode, knn.w_min,
                                 excl.off.data(), excl.nbr.data(), l.n_sel(), l.sel_ptr(), N, l.items.data(),
                                 l.scores.data(), l.count.data(), &st),
                     "cf_knn_topn");
    } else {
        src.ctx = cfcli::open_device();
        cfcli::check(src.ctx,
                     cf_mf_topn(src.ctx, nu, nm, src.fu.width, src.fu.F.data(), src.fv.F.data(),
                                bias ? src.bu.data() : nullptr, bias ? src.bi.data() : nullptr, mean,
                                matrix.empty() ? nullptr : excl.off.data(), matrix.empty() ? nullptr : excl.nbr.data(),
                                l.n_sel(), l.sel_ptr(), N, l.items.data(), l.scores.data(), l.count.data(), &st),
                     "cf_mf_topn");
    }
    cfrank::print_topn_stats(st);
    cfrank::write_lists(output, nshards, uids, mids, l);
    cf_destroy(src.ctx);
    return 0;
}
