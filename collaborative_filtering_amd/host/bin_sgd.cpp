// sgd -- drop-in for sgd.cpp: SGD matrix factorization of movielens/ ratings on the GPU.
// Everything is cfmf::sgd_main (cf_mf_cli.hpp), shared with biassgd.
#include "cf_mf_cli.hpp"

int main(int argc, char** argv) { return cfmf::sgd_main(argc, argv, false); }
