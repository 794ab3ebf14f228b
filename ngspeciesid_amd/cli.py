"""Command line of the reference (NGSpeciesID:187-287) over the MI355X hot path:  python -m ngspeciesid_amd --ont --fastq X --outfolder O --consensus --racon

Same flags and defaults, same output files (sorted.fastq, logfile.txt, final_clusters.tsv, final_cluster_origins.tsv,
consensus_reference_*.fasta, reads_to_consensus_*.fastq, racon_cl_id_*/consensus.fasta), including --primer_file /
--remove_universal_tails (barcode_trimmer.py).  --medaka is outside the hot path and is refused.
"""
from __future__ import annotations
import argparse, logging, os, sys


def main(args, api=None):
    """The CLI's work = the array path (fastpath.py).  The dict / file functions with the reference's Python signatures (cluster.reads_to_clusters, parallelize.parallel_clustering,
    consensus.run_spoa / run_racon / form_draft_consensus / polish_sequences) stay importable for callers of the reference's modules; tests/dict_layer.py drives them and compares
    the files they leave with the ones written here."""
    from . import fastpath
    return fastpath.main(args, api=api)


def write_fastq(args):
    """the `write_fastq` sub-command (NGSpeciesID:161-182, :238-245): one <cluster id>.fastq per cluster of final_clusters.tsv with at least --N reads.  The reference's
    semantics: the id and the accession are the first two white-space separated fields of a line, the reads are looked up by their WHOLE header line (an accession the FASTQ does
    not hold under that name is a KeyError, as there)."""
    from .help_functions import readfq, mkdir_p
    members = {}
    with open(args.clusters) as fh:
        for line in fh:
            f = line.split()
            if len(f) >= 2:
                members.setdefault(f[0], []).append(f[1])
    mkdir_p(args.outfolder)
    with open(args.fastq) as fh:
        record = {name: sq for name, sq in readfq(fh)}
    for cl_id, accs in members.items():
        if len(accs) < args.N:
            continue
        with open(os.path.join(args.outfolder, str(cl_id) + ".fastq"), "w") as out:
            for acc in accs:
                seq, qual = record[acc]
                out.write("@{0}\n{1}\n+\n{2}\n".format(acc, seq, qual))


FASTQ_DIR_NEEDS_T1 = ("--fastq_dir requires --t 1: with --t N the cluster membership depends on the batch schedule of every sample, and merge rounds are not "
                      "batched across samples. Run with --t 1, or run the samples one by one with --fastq.")

DEMUX_NEEDS_T1 = ("--demux_sheet requires --t 1: the demultiplexed samples are handed to the --fastq_dir path, where with --t N the cluster membership depends on the "
                  "batch schedule of every sample, and merge rounds are not batched across samples. Run with --t 1.")


def build_parser():
    p = argparse.ArgumentParser(description="Reference-free clustering and consensus forming of targeted ONT or PacBio reads (MI355X hot path)",
                                epilog="extension: `classify --fasta X --reference_db DB --outfile T` (first argument `classify`; `classify --help`) classifies the sequences of any FASTA against a reference library: the table of --reference_db; `chimeras --fasta X --outfile T` (first argument `chimeras`) writes the table of --chimeras for the sequences of any FASTA, taken as one sample; `variants --fasta A B ... --outfolder O` (first argument `variants`) writes the files of --variants with every FASTA taken as one sample; `recruit --fastq X --fasta CONS.fasta --outfolder O` (first argument `recruit`) writes the files of --recruit for any reads and any FASTA, taken as one sample; `umi --fastq X --outfolder O --umi_fwd PRE,POST --umi_rev PRE,POST` (first argument `umi`; `umi --help`) bins the reads of a UMI protocol by molecule and writes one polished consensus per bin",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--version', action='version', version='%(prog)s 0.3.1-mi355x')
    p.add_argument('--debug', action='store_true')
    rf = p.add_mutually_exclusive_group(required=True)
    rf.add_argument('--fastq', type=str)
    rf.add_argument('--use_old_sorted_file', action='store_true')
    rf.add_argument('--fastq_dir', type=str, help='extension: a folder of demultiplexed FASTQ files; every *.fastq / *.fq directly under it is one sample (sorted name order) and gets <outfolder>/<file name without extension>/ with the files a run of --fastq on it writes; all samples are clustered in one pass (needs --t 1)')
    p.add_argument('--t', dest="nr_cores", type=int, default=8, help='Number of score-ordered batches (the reference\'s cores); the cluster membership depends on it exactly like in the reference')
    p.add_argument('--d', dest="print_output", type=int, default=10000)
    p.add_argument('--q', dest="quality_threshold", type=float, default=7.0)
    p.add_argument('--ont', action="store_true"); p.add_argument('--isoseq', action="store_true")
    p.add_argument('--consensus', action="store_true")
    p.add_argument('--abundance_ratio', type=float, default=0.1)
    p.add_argument('--rc_identity_threshold', type=float, default=0.9)
    p.add_argument('--max_seqs_for_consensus', type=int, default=-1)
    g = p.add_mutually_exclusive_group()
    g.add_argument('--medaka', action="store_true"); g.add_argument('--racon', action="store_true")
    p.add_argument('--medaka_model', type=str, default=""); p.add_argument('--medaka_fastq', action="store_true")
    p.add_argument('--racon_iter', type=int, default=2)
    g2 = p.add_mutually_exclusive_group()
    g2.add_argument('--remove_universal_tails', action="store_true"); g2.add_argument('--primer_file', type=str, default="")
    p.add_argument('--primer_max_ed', type=int, default=2); p.add_argument('--trim_window', type=int, default=150)
    p.add_argument('--m', dest="target_length", type=int, default=0); p.add_argument('--s', dest="target_deviation", type=int, default=0)
    p.add_argument('--sample_size', type=int, default=0); p.add_argument('--top_reads', action='store_true')
    p.add_argument('--k', type=int, default=13); p.add_argument('--w', type=int, default=20)
    p.add_argument('--min_shared', type=int, default=5); p.add_argument('--mapped_threshold', type=float, default=0.7)
    p.add_argument('--aligned_threshold', type=float, default=0.4); p.add_argument('--symmetric_map_align_thresholds', action='store_true')
    p.add_argument('--batch_type', type=str, default='total_nt'); p.add_argument('--min_fraction', type=float, default=0.8)
    p.add_argument('--min_prob_no_hits', type=float, default=0.1); p.add_argument('--outfolder', type=str, default=None)
    # extensions of this build (not in the reference): shape of the consensus engine.  Defaults = the measured configuration.
    p.add_argument('--poa_tile_depth', type=int, default=4, help='reads per exact-order POA tile (default 4: depth-tiled hierarchy; a positive value also applies to the polishing windows). 0 = one graph per cluster in read order, i.e. spoa\'s order; a graph holds at most 65 520 nodes, so use it with --max_seqs_for_consensus (a few hundred reads); larger clusters are split by the capacity rule')
    p.add_argument('--strand_aware', action='store_true', help='extension: clusters whose representatives are reverse complements of each other (decided by the clustering criteria themselves) are joined BEFORE the consensus stage and their reads are oriented: one cluster per amplicon in final_clusters.tsv; off = the reference (two clusters per amplicon on mixed-strand data, joined after the drafts)')
    p.add_argument('--polish_all_iterations', action='store_true', help='extension: run every --racon_iter iteration even when an iteration returned its input unchanged (the default stops polishing such a cluster: same result, less time)')
    p.add_argument('--poa_single_below', type=int, default=None, help='extension: clusters / polishing windows with fewer sequences than this are aligned as ONE graph in read order (spoa\'s and racon\'s own order) instead of being depth-tiled; 0 = tile everything; default: the library\'s measured threshold (pipeline.SINGLE_BELOW)')
    p.add_argument('--racon_subgraph_layers', action='store_true', help='extension: a polishing layer that does not span its window is aligned globally to the sub-graph between its first and last backbone positions, as racon does, instead of end-free to the whole window graph (default off: the shipped polisher)')
    p.add_argument('--consensus_support', action='store_true', help='extension: per-base read support of every consensus. Writes racon_cl_id_*/consensus.fastq (header and sequence of consensus.fasta, qualities from the support as Phred+33) and racon_cl_id_*/consensus_support.tsv (pos base depth agree A C G T del ins_after); without --racon, consensus_reference_{id}.fastq and consensus_reference_{id}.support.tsv')
    p.add_argument('--demux_sheet', type=str, default=None, help='extension: --fastq is a pooled run; FILE is a TSV with one row per sample, sample<TAB>forward tag[<TAB>reverse tag] (tags of up to 64 bases, IUPAC codes allowed, primer included if wanted). Every read end is searched for every tag on the GPU; the reads are written to <outfolder>/demux/<sample>.fastq (+ <outfolder>/demux_unassigned.fastq, <outfolder>/demux_summary.tsv) and the samples then run like --fastq_dir <outfolder>/demux (needs --fastq, --outfolder and --t 1)')
    p.add_argument('--demux_max_ed', type=int, default=3, help='extension: largest edit distance at which a tag counts as found in a read end')
    p.add_argument('--demux_window', type=int, default=150, help='extension: bases of each read end that are searched for the tags (1..256)')
    p.add_argument('--demux_min_margin', type=int, default=2, help='extension: an end is ambiguous when its second-best tag is closer than this many edits to its best')
    p.add_argument('--demux_keep_tags', action='store_true', help='extension: leave the tags on the demultiplexed reads (default: cut each end behind its tag)')
    p.add_argument('--demux_only', action='store_true', help='extension: stop after the demultiplexing outputs')
    p.add_argument('--demux_mid_tags', type=str, default='off', choices=['off', 'discard', 'split'], help='extension: search the WHOLE read for the sheet\'s tags on both strands (GPU) and treat a read with a tag inside as a concatemer. discard: it goes whole to demux_unassigned.fastq with status mid_tag. split: it is cut at the tags and every piece is demultiplexed once more (pieces are named <read>/p<k>). Writes <outfolder>/demux_concatemers.tsv and extra lines in demux_summary.tsv (default off)')
    p.add_argument('--demux_mid_max_ed', type=int, default=None, help='extension: largest edit distance at which a tag counts as found inside a read (default: by tag length, 1 from 13 bases, 2 from 16, 3 from 24, 0 below - profiles/demux.txt)')
    p.add_argument('--reference_db', type=str, default=None, help='extension: FASTA of reference barcodes (BOLD, UNITE, SILVA, ...). Every final consensus (the polished one with --racon, else the draft) is searched in it on the GPU by shared minimizers, both strands, and its best candidates are verified by alignment; writes <outfolder>/classification.tsv (consensus_id n_reads rank reference strand shared identity aln_cols n_match q_cov r_cov called header; with --fastq_dir / --demux_sheet one table per sample folder and <outfolder>/classification_all.tsv). Needs --consensus')
    from . import classify as _classify
    _classify.add_flags(p)
    from . import chimera as _chimera
    p.add_argument('--chimeras', action='store_true', help='extension: flag PCR chimeras among the final consensuses. Every consensus is modelled on the GPU as the head of one and the tail of another more abundant consensus of the same sample (both strands, unit-cost edit distance, every breakpoint); writes <outfolder>/chimeras.tsv (id n_reads length chimeric best_parent best_strand best_ed parent_a strand_a parent_b strand_b model_ed gain bp_lo bp_hi; with --fastq_dir / --demux_sheet one table per sample folder and <outfolder>/chimeras_all.tsv). No other output changes. Needs --consensus')
    _chimera.add_flags(p)
    from . import variants as _variants
    p.add_argument('--variants', action='store_true', help='extension: the study-wide variant table of a multi-sample run. The final consensuses of all samples are compared with each other on the GPU (banded unit-cost edit distance, both strands) and joined by abundance into variants; writes <outfolder>/variants.fasta (the centroid sequences, variant_{v};size={reads};samples={n}), variant_table.tsv (variants x samples, read counts) and variant_members.tsv (sample, consensus id, reads, variant, dist, strand). No other output changes. Needs --consensus and --fastq_dir or --demux_sheet')
    _variants.add_flags(p)
    from . import hp as _hp
    p.add_argument('--hp_polish', action='store_true', help='extension: homopolymer finishing pass, a run-length vote and NOT medaka (--medaka stays refused: no neural polisher). For every homopolymer run of every final consensus (the polished one with --racon, else the draft) the GPU counts, per strand, how long that run is in every read that spans it between two matching flanks; a run is rewritten to the length most reads carry when the thresholds below are met. Letters never change and no run is removed. The consensus files carry the corrected sequence; writes <outfolder>/hp_polish.tsv (cluster_id pos letter old_len new_len round hist_plus hist_minus; with --fastq_dir / --demux_sheet one table per sample folder and <outfolder>/hp_polish_all.tsv). Support, classification, chimeras and haplotypes see the corrected sequences. Needs --consensus')
    p.add_argument('--hp_rounds', type=int, default=2, help='extension: rounds of --hp_polish; a further round runs only on the consensuses the round before changed')
    p.add_argument('--hp_min_depth', type=int, default=_hp.DEFAULTS["min_depth"], help='extension: --hp_polish calls a length only when at least this many reads give one (both strands)')
    p.add_argument('--hp_min_share', type=float, default=_hp.DEFAULTS["min_share"], help='extension: the called length holds at least this share of those reads')
    p.add_argument('--hp_min_margin', type=float, default=_hp.DEFAULTS["min_margin"], help="extension: and leads the consensus's own length by at least this share of them")
    p.add_argument('--hp_min_strand_depth', type=int, default=_hp.DEFAULTS["min_strand_depth"], help="extension: a strand with at least this many reads of its own that does not prefer the called length to the consensus's vetoes the call")
    from . import recruit as _recruit
    p.add_argument('--recruit', action='store_true', help='extension: recruit every read of the sample to its nearest final consensus. Every read of sorted.fastq is located on the GPU inside every final consensus (the consensus end to end, the read\'s ends free, both strands, unit-cost edit distance) and counts for the nearest one within the identity bound; writes <outfolder>/recount.tsv (consensus reads_clustered reads_recruited from_own_clusters from_other_centres from_unclustered, then the ambiguous and unassigned totals) and read_assignments.tsv (read consensus strand ed identity status; with --fastq_dir / --demux_sheet both per sample folder and <outfolder>/recount_all.tsv). No other output changes. Needs --consensus')
    _recruit.add_flags(p)
    from . import sam as _sam
    _sam.add_flags(p)
    from . import errprof as _errprof
    _errprof.add_flags(p)
    from . import phase as _phase
    p.add_argument('--split_haplotypes', action='store_true', help='extension: split every cluster whose reads carry linked variant sites (two alleles, a NUMT beside its original, sister species) into haplotypes. Sites come from the per-base support, the read x site genotypes, pair tables and the assignment are computed on the GPU; every haplotype gets its own draft and polish. Writes <outfolder>/haplotypes.tsv (cluster_id haplotype reads sites alleles) and racon_cl_id_{id}/consensus_h{j}.fasta (without --racon consensus_reference_{id}_h{j}.fasta); with --reference_db the haplotypes are rows of classification.tsv. Needs --consensus; not with --fastq_dir / --demux_sheet')
    p.add_argument('--hap_min_alt_frac', type=float, default=_phase.DEFAULTS["min_alt_frac"], help='extension: a base is a candidate site when its second most frequent allele holds at least this share of the depth')
    p.add_argument('--hap_min_reads', type=int, default=_phase.DEFAULTS["min_hap_reads"], help='extension: an allele string is a haplotype when at least this many reads carry it')
    p.add_argument('--hap_min_phi', type=float, default=_phase.DEFAULTS["min_phi"], help='extension: two sites are linked at this phi coefficient of their allele table or above')
    p.add_argument('--hap_max', type=int, default=_phase.DEFAULTS["max_haps"], help='extension: most haplotypes per cluster (2..16)')
    p.add_argument('--skip_paf', action='store_true', help='extension: do not write racon_cl_id_*/read_alignments_it_{i}.paf (the reference leaves minimap2\'s PAF of every polishing iteration there; default: written)')
    p.set_defaults(which='main')
    sub = p.add_subparsers(help='sub-command help')
    wf = sub.add_parser('write_fastq', help='write the reads of every cluster of final_clusters.tsv to <outfolder>/<cluster id>.fastq (NGSpeciesID:238-245)')
    wf.add_argument('--clusters', type=str, help='final_clusters.tsv of a run')
    wf.add_argument('--fastq', type=str, help='Input fastq file')
    wf.add_argument('--outfolder', type=str, help='Output folder')
    wf.add_argument('--N', type=int, default=0, help='Write out clusters with more or equal than N reads')
    wf.set_defaults(which='write_fastq')
    p.add_argument('--poa_band', type=int, default=0, help='band of the POA alignments in columns (0 = library default: 64 for reads up to 3 kb, else 128; a tile whose path touches the band edge is redone at twice the band)')
    return p


def _classify_subparser(cf):
    """the `classify` sub-command.  It is parsed by a parser of its own (cli() below), not as a sub-parser of the main command like write_fastq: the main command requires one
    of --fastq / --use_old_sorted_file / --fastq_dir, which a sub-parser cannot lift, and `classify --fasta X --reference_db DB --outfile T` needs none of them."""
    from . import classify as _classify
    cf.add_argument('--fasta', type=str, required=True, help='sequences to classify')
    cf.add_argument('--reference_db', type=str, required=True, help='FASTA of reference barcodes')
    cf.add_argument('--outfile', type=str, required=True, help='the table (columns of classification.tsv)')
    _classify.add_flags(cf)
    cf.set_defaults(which='classify')
    return cf


def _chimeras_subparser(cf):
    """the `chimeras` sub-command: parsed by a parser of its own, like `classify`"""
    from . import chimera as _chimera
    cf.add_argument('--fasta', type=str, required=True, help='sequences of one sample; read counts are taken from names of this tool\'s consensuses (..._total_supporting_reads_N), else 0')
    cf.add_argument('--outfile', type=str, required=True, help='the table (columns of chimeras.tsv)')
    _chimera.add_flags(cf)
    cf.set_defaults(which='chimeras')
    return cf


def _variants_subparser(cf):
    """the `variants` sub-command: parsed by a parser of its own, like `classify`"""
    from . import variants as _variants
    cf.add_argument('--fasta', type=str, nargs='+', required=True, help='one FASTA per sample (the sample is named by the file name without its extension); read counts are taken from names of this tool\'s consensuses (..._total_supporting_reads_N), else 1')
    cf.add_argument('--outfolder', type=str, required=True, help='where variants.fasta, variant_table.tsv and variant_members.tsv go')
    _variants.add_flags(cf)
    cf.set_defaults(which='variants')
    return cf


def _umi_subparser(cf):
    """the `umi` sub-command: parsed by a parser of its own, like `classify`"""
    from . import umi as _umi
    cf.add_argument('--fastq', type=str, required=True, help='reads of a UMI protocol: adapter - flank - UMI - primer - amplicon - primer\' - UMI\' - flank\'')
    cf.add_argument('--outfolder', type=str, required=True, help='where umi_consensus.fasta, umi_bins.tsv, umi_reads.tsv and umi_summary.tsv go')
    _umi.add_flags(cf)
    cf.set_defaults(which='umi')
    return cf


def _recruit_subparser(cf):
    """the `recruit` sub-command: parsed by a parser of its own, like `classify`"""
    from . import recruit as _recruit
    cf.add_argument('--fastq', type=str, required=True, help='the reads')
    cf.add_argument('--fasta', type=str, required=True, help='the sequences the reads are recruited to, taken as one sample (at most 2048 letters each); read counts are taken from names of this tool\'s consensuses (..._total_supporting_reads_N), else 0')
    cf.add_argument('--outfolder', type=str, required=True, help='where recount.tsv and read_assignments.tsv go')
    cf.add_argument('--q', dest="quality_threshold", type=float, default=7.0, help='the read filter of the run the reads come from: the default of --recruit_min_identity')
    _recruit.add_flags(cf)
    cf.set_defaults(which='recruit')
    return cf


def _sam_subparser(cf):
    """the `sam` sub-command: parsed by a parser of its own, like `classify`"""
    from . import recruit as _recruit
    cf.add_argument('--fastq', type=str, required=True, help='the reads')
    cf.add_argument('--fasta', type=str, required=True, help='the sequences the reads are recruited and aligned to (at most 2048 letters each): every one is a target of the file')
    cf.add_argument('--outfile', type=str, required=True, help='the SAM file: assigned reads mapped to their sequence (CIGAR with = and X, NM tag), all other reads unmapped')
    cf.add_argument('--q', dest="quality_threshold", type=float, default=7.0, help='the read filter of the run the reads come from: the default of --recruit_min_identity')
    cf.add_argument('--sam_merge_m', action='store_true', help='write M instead of = and X')
    _recruit.add_flags(cf)
    cf.set_defaults(which='sam')
    return cf


def _errprof_subparser(cf):
    """the `errprof` sub-command: parsed by a parser of its own, like `classify`"""
    from . import recruit as _recruit
    cf.add_argument('--fastq', type=str, required=True, help='the reads')
    cf.add_argument('--fasta', type=str, required=True, help='the sequences the reads are recruited to and profiled against (at most 2048 letters each)')
    cf.add_argument('--outfolder', type=str, required=True, help='where error_profile.tsv and quality_calibration.tsv go')
    cf.add_argument('--q', dest="quality_threshold", type=float, default=7.0, help='the read filter of the run the reads come from: the default of --recruit_min_identity')
    _recruit.add_flags(cf)
    cf.set_defaults(which='errprof')
    return cf


def _check_recruit(args):
    from . import recruit as _recruit
    err = _recruit.check_args(args)
    if err:
        logging.error(err); sys.exit(1)


def _check_variants(args):
    from . import variants as _variants
    err = _variants.check_args(args)
    if err:
        logging.error(err); sys.exit(1)


def _check_chimeras(args):
    from . import chimera as _chimera
    err = _chimera.check_args(args)
    if err:
        logging.error(err); sys.exit(1)


def _check_classify(args):
    from . import classify as _classify
    err = _classify.check_args(args)
    if err:
        logging.error(err); sys.exit(1)
    if not os.path.isfile(args.reference_db):
        logging.error("--reference_db %s is not a file." % args.reference_db); sys.exit(1)


def cli(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if argv and argv[0] == 'classify':              # `classify --fasta X --reference_db DB --outfile T` needs none of the main command's inputs
        args = _classify_subparser(argparse.ArgumentParser(prog='classify', formatter_class=argparse.ArgumentDefaultsHelpFormatter)).parse_args(argv[1:])
    elif argv and argv[0] == 'chimeras':
        args = _chimeras_subparser(argparse.ArgumentParser(prog='chimeras', formatter_class=argparse.ArgumentDefaultsHelpFormatter)).parse_args(argv[1:])
    elif argv and argv[0] == 'variants':
        args = _variants_subparser(argparse.ArgumentParser(prog='variants', formatter_class=argparse.ArgumentDefaultsHelpFormatter)).parse_args(argv[1:])
    elif argv and argv[0] == 'recruit':
        args = _recruit_subparser(argparse.ArgumentParser(prog='recruit', formatter_class=argparse.ArgumentDefaultsHelpFormatter)).parse_args(argv[1:])
    elif argv and argv[0] == 'sam':
        args = _sam_subparser(argparse.ArgumentParser(prog='sam', formatter_class=argparse.ArgumentDefaultsHelpFormatter)).parse_args(argv[1:])
    elif argv and argv[0] == 'errprof':
        args = _errprof_subparser(argparse.ArgumentParser(prog='errprof', formatter_class=argparse.ArgumentDefaultsHelpFormatter)).parse_args(argv[1:])
    elif argv and argv[0] == 'umi':
        args = _umi_subparser(argparse.ArgumentParser(prog='umi', formatter_class=argparse.ArgumentDefaultsHelpFormatter)).parse_args(argv[1:])
    else:
        args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if getattr(args, 'debug', False) else logging.INFO, format='%(message)s')
    if getattr(args, "which", "main") == 'write_fastq':          # NGSpeciesID:255-258
        write_fastq(args)
        logging.info("Wrote clusters to separate fastq files.")
        sys.exit(0)
    if getattr(args, "which", "main") == 'classify':
        _check_classify(args)
        from . import classify as _classify
        rows = _classify.classify_fasta(args)
        logging.info("Wrote %d rows to %s." % (len(rows), args.outfile))
        sys.exit(0)
    if getattr(args, "which", "main") == 'chimeras':
        _check_chimeras(args)
        if not os.path.isfile(args.fasta):
            logging.error("--fasta %s is not a file." % args.fasta); sys.exit(1)
        from . import chimera as _chimera
        rows = _chimera.chimeras_fasta(args)
        logging.info("Wrote %d rows to %s." % (len(rows), args.outfile))
        sys.exit(0)
    if getattr(args, "which", "main") == 'variants':
        _check_variants(args)
        for f in args.fasta:
            if not os.path.isfile(f):
                logging.error("--fasta %s is not a file." % f); sys.exit(1)
        from . import variants as _variants
        tab = _variants.variants_fasta(args)
        logging.info("Wrote %d variants of %d sequences to %s." % (len(tab["variants"]), len(tab["members"]), args.outfolder))
        sys.exit(0)
    if getattr(args, "which", "main") == 'recruit':
        _check_recruit(args)
        for f in (args.fastq, args.fasta):
            if not os.path.isfile(f):
                logging.error("%s is not a file." % f); sys.exit(1)
        from . import recruit as _recruit
        res = _recruit.recruit_fastq(args)
        logging.info("Recruited %d of %d reads to %d sequences; wrote %s." % (int((res["status"] == _recruit.ASSIGNED).sum()), len(res["status"]), len(res["counts"]["centres"]), args.outfolder))
        sys.exit(0)
    if getattr(args, "which", "main") == 'sam':
        _check_recruit(args)
        for f in (args.fastq, args.fasta):
            if not os.path.isfile(f):
                logging.error("%s is not a file." % f); sys.exit(1)
        from . import sam as _sam
        res = _sam.sam_fastq(args)
        logging.info("Wrote %d records (%d mapped) to %s." % (res["records"], res["mapped"], args.outfile))
        sys.exit(0)
    if getattr(args, "which", "main") == 'errprof':
        _check_recruit(args)
        for f in (args.fastq, args.fasta):
            if not os.path.isfile(f):
                logging.error("%s is not a file." % f); sys.exit(1)
        from . import errprof as _errprof
        res = _errprof.errprof_fastq(args)
        logging.info("Profiled %d reads against %d sequences; wrote %s." % (sum(len(l) for l in res["lists"]), len(res["ids"]), args.outfolder))
        sys.exit(0)
    if getattr(args, "which", "main") == 'umi':
        from . import umi as _umi
        err = _umi.check_args(args)
        if err:
            logging.error(err); sys.exit(1)
        if not os.path.isfile(args.fastq):
            logging.error("--fastq %s is not a file." % args.fastq); sys.exit(1)
        res = _umi.umi_fastq(args)
        logging.info("Wrote %d UMI consensus sequences of %d bins (%d reads) to %s." % (len(res["kept"]), len(res["bins"]["centroids"]), len(res["status"]), args.outfolder))
        sys.exit(0)
    if args.ont and args.isoseq:
        logging.error("Arguments mutually exclusive, specify either --isoseq or --ont. "); sys.exit()
    elif args.isoseq:
        args.k, args.w = 15, 50
    elif args.ont:
        args.k, args.w = 13, 20
    if getattr(args, "split_haplotypes", False):
        if getattr(args, "fastq_dir", None) or getattr(args, "demux_sheet", None):
            logging.error("--split_haplotypes works on one sample: it cannot be combined with --fastq_dir or --demux_sheet (run the samples one by one)."); sys.exit(1)
        if not args.consensus:
            logging.error("--split_haplotypes splits the reads of consensus sequences: it needs --consensus."); sys.exit(1)
        from . import phase as _phase
        err = _phase.check_args(args)
        if err:
            logging.error(err); sys.exit(1)
    if getattr(args, "fastq_dir", None):
        if args.nr_cores != 1:
            logging.error(FASTQ_DIR_NEEDS_T1); sys.exit(1)
        if not args.outfolder:
            logging.error("--fastq_dir needs --outfolder (one sub-folder per sample is written there)."); sys.exit(1)
        if not os.path.isdir(args.fastq_dir):
            logging.error("--fastq_dir %s is not a folder." % args.fastq_dir); sys.exit(1)
    if getattr(args, "demux_sheet", None):
        if getattr(args, "fastq_dir", None) or args.use_old_sorted_file or not args.fastq:
            logging.error("--demux_sheet splits ONE pooled file: give it with --fastq, not with --fastq_dir or --use_old_sorted_file."); sys.exit(1)
        if args.nr_cores != 1:
            logging.error(DEMUX_NEEDS_T1); sys.exit(1)
        if not args.outfolder:
            logging.error("--demux_sheet needs --outfolder (the sample files and one sub-folder per sample are written there)."); sys.exit(1)
        if not os.path.isfile(args.demux_sheet):
            logging.error("--demux_sheet %s is not a file." % args.demux_sheet); sys.exit(1)
        if not 1 <= args.demux_window <= 256 or args.demux_max_ed < 0 or args.demux_min_margin < 0:
            logging.error("--demux_window must be 1..256, --demux_max_ed and --demux_min_margin must not be negative."); sys.exit(1)
        if args.demux_mid_max_ed is not None and args.demux_mid_max_ed < 0:
            logging.error("--demux_mid_max_ed must not be negative."); sys.exit(1)
        if args.demux_mid_max_ed is not None and args.demux_mid_tags == 'off':
            logging.error("--demux_mid_max_ed is the edit bound of --demux_mid_tags discard | split."); sys.exit(1)
    elif getattr(args, "demux_mid_tags", "off") != 'off' or getattr(args, "demux_mid_max_ed", None) is not None:
        logging.error("--demux_mid_tags and --demux_mid_max_ed need --demux_sheet."); sys.exit(1)
    if getattr(args, "reference_db", None):
        if not args.consensus:
            logging.error("--reference_db classifies consensus sequences: it needs --consensus."); sys.exit(1)
        _check_classify(args)
    if getattr(args, "chimeras", False):
        if not args.consensus:
            logging.error("--chimeras models consensus sequences: it needs --consensus."); sys.exit(1)
        _check_chimeras(args)
    if getattr(args, "variants", False):
        if not args.consensus:
            logging.error("--variants joins consensus sequences: it needs --consensus."); sys.exit(1)
        if not (getattr(args, "fastq_dir", None) or getattr(args, "demux_sheet", None)):
            logging.error("--variants joins the consensuses of several samples: it needs --fastq_dir or --demux_sheet."); sys.exit(1)
        _check_variants(args)
    if getattr(args, "recruit", False):
        if not args.consensus:
            logging.error("--recruit recruits reads to consensus sequences: it needs --consensus."); sys.exit(1)
        _check_recruit(args)
    if getattr(args, "write_sam", False) or getattr(args, "sam_merge_m", False):
        from . import sam as _sam
        err = _sam.check_args(args) or (None if args.consensus else "--write_sam aligns reads to consensus sequences: it needs --consensus.")
        if err:
            logging.error(err); sys.exit(1)
    if getattr(args, "error_profile", False) and not args.consensus:
        logging.error("--error_profile profiles reads against consensus sequences: it needs --consensus."); sys.exit(1)
    if getattr(args, "hp_polish", False):
        if not args.consensus:
            logging.error("--hp_polish corrects consensus sequences: it needs --consensus."); sys.exit(1)
        if args.hp_rounds < 1 or args.hp_min_depth < 1 or not (0.0 <= args.hp_min_share <= 1.0) or not (0.0 <= args.hp_min_margin <= 1.0) or args.hp_min_strand_depth < 1:
            logging.error("--hp_rounds, --hp_min_depth and --hp_min_strand_depth are at least 1, --hp_min_share and --hp_min_margin lie in [0, 1]."); sys.exit(1)
    if args.medaka:
        logging.error("--medaka (neural polisher) is outside the accelerated hot path (see DESIGN.md); use --racon, and --hp_polish for a run-length vote on the homopolymers."); sys.exit(1)
    if args.k > 32 or args.k < 1:
        logging.error('k = %d is outside what the minimizer encoder of this build handles (1..32; the shared-minimizer table has rows for k = 10..30).' % args.k); sys.exit(1)
    if 100 < args.w or args.w < args.k:
        logging.error('Please specify a window of size larger or equal to k, and smaller than 100.'); sys.exit(1)
    if args.poa_single_below is None:
        from . import pipeline
        args.poa_single_below = pipeline.SINGLE_BELOW
    if args.outfolder and not os.path.exists(args.outfolder):
        os.makedirs(args.outfolder)
    main(args)


if __name__ == "__main__":
    cli()
