// biassgd -- drop-in for biassgd.cpp: SGD with user / item biases and the global mean on the GPU.
// Everything is cfmf::sgd_main (cf_mf_cli.hpp), shared with sgd.
#include "cf_mf_cli.hpp"

int main(int argc, char** argv) { return cfmf::sgd_main(argc, argv, true); }
