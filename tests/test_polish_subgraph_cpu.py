"""NGSID_ALN_SUBGRAPH (racon's sub-graph alignment of the window layers that do not span their window): the parameter plumbing of the Python layer and the CLI.
The polisher itself is compared with the oracle in tests/test_gpu_polish_subgraph.py."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ngspeciesid_amd import cli, fastpath, pipeline
from ngspeciesid_amd._capi import polish_params, ALN_SUBGRAPH

FIELDS = [f[0] for f in polish_params()._fields_]


def test_flag_bit_of_aln_mode():
    assert ALN_SUBGRAPH == 16
    for mode in (0, 1, 2, 3):
        assert polish_params(aln_mode=mode, subgraph_layers=True).aln_mode == mode | 16
        assert polish_params(aln_mode=mode).aln_mode == mode
    assert polish_params(subgraph_layers=True).aln_mode & 16


def _args(extra):
    args = cli.build_parser().parse_args(["--ont", "--fastq", "x.fastq", "--outfolder", "o", "--racon"] + extra)
    args.k, args.w = 13, 20
    return args


def test_cli_flag_parses():
    assert _args([]).racon_subgraph_layers is False
    assert _args(["--racon_subgraph_layers"]).racon_subgraph_layers is True
    assert "--racon_subgraph_layers" in cli.build_parser().format_help()


def test_cli_polish_parameters_carry_the_bit_only_with_the_flag():
    for extra in ([], ["--racon_iter", "3", "--poa_tile_depth", "6", "--poa_band", "128", "--polish_all_iterations", "--poa_single_below", "10"]):
        for clip in (False, True):
            for node_cap in (0, 22):
                off = fastpath._polish_prm(_args(extra), node_cap, clip)
                on = fastpath._polish_prm(_args(extra + ["--racon_subgraph_layers"]), node_cap, clip)
                assert off.aln_mode == (3 if clip else 2) and on.aln_mode == off.aln_mode | 16
                assert off.trim == (3 if clip else 2)
                for f in FIELDS:
                    if f != "aln_mode": assert getattr(on, f) == getattr(off, f), f
                # the expression the CLI used before the helper existed
                a = _args(extra)
                old = polish_params(iters=a.racon_iter, k=a.k, w=a.w, tile_depth=(a.poa_tile_depth if a.poa_tile_depth > 0 else pipeline.TILE_DEPTH), band=a.poa_band, node_cap=node_cap,
                                    trim=3 if clip else 2, aln_mode=3 if clip else 2, stop_when_stable=0 if a.polish_all_iterations else 1, single_below=fastpath._single_below(a))
                for f in FIELDS:
                    assert getattr(off, f) == getattr(old, f), f
