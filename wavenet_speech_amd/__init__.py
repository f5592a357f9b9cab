"""
wavenet_speech_amd -- MI355X-native WaveNet dilated residual-block stack behind the nn.Module surface of
paultsw/wavenet-speech (modules.wavenet.WaveNet, modules.raw_ctcnet.RawCTCNet, modules.block.ResidualBlock,
modules.classifier.WaveNetClassifier, modules.conv_ops.*).

    from wavenet_speech_amd.modules.wavenet import WaveNet      # instead of: from modules.wavenet import WaveNet

All arithmetic of the hot path runs in hand-written HIP kernels (csrc/, gfx950) reached through the C ABI of
libwavenet_amd.so (include/wavenet_amd.h).  No CPU fallback exists.
"""
from . import basecalling, decoding, demux, events, functional, graphs, mapping, modules, normalise, readmap, series  # noqa: F401
from .modules import (CausalConv1d, NonCausalConv1d, RawCTCNet, ResidualBlock, WaveNet,  # noqa: F401
                      WaveNetClassifier)
from .modules.block import freeze_for_inference, set_precision  # noqa: F401
from ._flags import check_device_flags  # noqa: F401
from .graphs import GraphedStep  # noqa: F401
from .decoding import (BaseQualities, CTCAlignment, CTCBeamDecoder, PairwiseAlignment, QualityCalibration,  # noqa: F401
                       QualityProfile, ctc_base_qualities, ctc_beam_decode, ctc_forced_align, ctc_greedy_decode, edit_distance,
                       fastq_records, fit_quality_calibration, format_alignment, labels_to_strings, pairwise_align,
                       quality_profile)
from .decoding import BandedAlignment, band_from_ops, banded_align  # noqa: F401
from .functional_half import check_fp16_overflow  # noqa: F401
from .basecalling import Basecaller, Basecalls, ChunkPlan, chunk_plan, receptive_field  # noqa: F401
from .normalise import read_med_mad, read_normalisation, read_order_statistics, read_quantiles  # noqa: F401
from .events import KmerEvents, eventalign_rows, fit_dwell_model, fit_kmer_model, kmer_events  # noqa: F401
from .events import SignalAlignment, SignalModel, signal_align, signal_model  # noqa: F401
from .events import DetectedEvents, detect_events  # noqa: F401
from .events import DEFAULT_MOVES, EventAlignment, event_align, fit_moves, move_costs  # noqa: F401
from .demux import (BarcodeSet, Demultiplexed, DemuxScores, demultiplex, demux_scores, reverse_complement,  # noqa: F401
                    trim_reads)
from .readmap import (Anchors, Minimizers, ReadIndex, ReadMapping, chain_anchors, map_reads, minimizers, paf_records,  # noqa: F401
                      read_index, seed_anchors)
from .pileup import ConsensusCalls, Pileup, Variant, call_consensus, pileup, variant_records, vcf_records  # noqa: F401
from .leftalign import LeftAligned, left_align  # noqa: F401
from .genotype import (Evidence, GenotypeRecord, Genotypes, GenotypeWeights, call_genotypes, genotype_records, genotype_weights,  # noqa: F401
                       pileup_evidence, vcf_genotype_records)
from .phase import (Haplotags, PhasedRecord, PhaseLinks, PhaseSites, Phasing, haplotag, phase_chain, phase_links, phase_sites,  # noqa: F401
                    phased_records, vcf_phased_records)
from .realign import (HaplotypeCalls, HaplotypeWindows, Realignment, haplotype_calls, haplotype_windows, lift_alignment,  # noqa: F401
                      realign)
from .sam import (CigarAlignment, CigarRows, SamReads, cigar_ops, cigar_runs, cigar_strings, md_strings, parse_sam, sam_header,  # noqa: F401
                  sam_records)
from .mapping import MapReference, SignalMapping, join_strands, map_reference, signal_map  # noqa: F401
from .synthetic import RaggedReads, RawGaussianModelLoader, ragged_reads  # noqa: F401

__version__ = "0.1.0"
