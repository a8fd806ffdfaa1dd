"""graph-normalizing-flows_amd: MI355X (gfx950) implementation of the GRevNet forward / inverse +
log-det hot path of jliu/graph-normalizing-flows behind the reference's own gnn.py call surface.

Import as `gnf_amd` (the directory name has a hyphen; gnf_amd.py at the repo root is the loader):
    from gnf_amd.gnn import GRevNet, avg_then_mlp_gnn, make_mlp_model, leaky_relu
    from gnf_amd.flow import log_prob_per_graph, sample, decode_graphs, generate_graphs
    from gnf_amd.graph_stats import graph_stats, hist_mmd, evaluate_generated, graph_orbits, orbit_mmd, graph_spectra, spectral_mmd
    from gnf_amd.graph_stats import graph_components, keep_subgraphs, graph_hashes, uniqueness_novelty
    from gnf_amd.adj_loss import binary_loss, hacky_sigmoid_l2, sigmoid_l2, TunedSigmoidL2, incorrect_edges_per_graph
    from gnf_amd.adj_loss import reconstruction_report, predicted_graph, error_graph
    from gnf_amd.triplet_loss import triplet_loss, l2, exp_l2, margin_loss, relative_loss
    from gnf_amd.gnn import TimestepGNN
    from gnf_amd.encoder import evaluate, write_embedding_chunks
    from gnf_amd.train import EncoderTrainer
"""
from . import _abi
from .graphs import GraphsTuple, data_dicts_to_graphs_tuple, build_csr_host, csr_of, seed_csr_cache
from .graph_stats import graph_stats, hist_mmd, evaluate_generated, graph_orbits, orbit_mmd, graph_spectra, spectral_mmd
from .graph_stats import graph_components, keep_subgraphs, graph_hashes, uniqueness_novelty
from .adj_loss import (binary_loss, hacky_sigmoid_l2, sigmoid_l2, TunedSigmoidL2, incorrect_edges_per_graph,
                       false_positive_edges, false_negative_edges, total_incorrect_edges, reconstruction_report,
                       predicted_graph, error_graph)
from .triplet_loss import triplet_loss, margin_loss, relative_loss
from .gnn import TimestepGNN
from .encoder import evaluate, write_embedding_chunks
from .train import EncoderTrainer, encoder_learning_rate, encoder_trainer_state, load_encoder_trainer_state

__all__ = ["GraphsTuple", "data_dicts_to_graphs_tuple", "build_csr_host", "csr_of", "seed_csr_cache", "_abi",
           "graph_stats", "hist_mmd", "evaluate_generated", "graph_orbits", "orbit_mmd", "graph_spectra", "spectral_mmd",
           "graph_components", "keep_subgraphs", "graph_hashes", "uniqueness_novelty",
           "binary_loss", "hacky_sigmoid_l2", "sigmoid_l2", "TunedSigmoidL2", "incorrect_edges_per_graph", "false_positive_edges",
           "false_negative_edges", "total_incorrect_edges", "reconstruction_report", "predicted_graph", "error_graph",
           "triplet_loss", "margin_loss", "relative_loss", "TimestepGNN", "evaluate", "write_embedding_chunks",
           "EncoderTrainer", "encoder_learning_rate", "encoder_trainer_state", "load_encoder_trainer_state"]
