"""Host-side mirror of the reference's Java API over the C ABI of libbwamem_hip.so.

The reference host is Java (src/main/java/org/broadinstitute/hellbender/utils/bwa/); no JDK
exists in this build environment, so the same operator interface is mirrored here -- same
class and method names, argument meaning and error behaviour -- so that tests read like
BwaMemIndexTest.java.  The Java classes themselves stay unchanged and bind the very same
library through the JNI glue.

  BwaMemIndex          <- BwaMemIndex.java:29-488
  BwaMemAligner        <- BwaMemAligner.java:20-327
  BwaMemAlignment      <- BwaMemAlignment.java:8-65
  BwaMemPairEndStats   <- BwaMemPairEndStats.java:15-205

The library is the product: if libbwamem_hip.so is missing this module fails to import.
"""
import ctypes
import math
import os
import struct
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("LIBBWA_PATH", os.path.join(_HERE, "libbwamem_hip.so"))   # BwaMemIndex.java:438-441
if not os.path.exists(_LIB_PATH):
    raise ImportError("native library %s not found: build it with __graft_entry__.build()" % _LIB_PATH)
_lib = ctypes.CDLL(_LIB_PATH)

_lib.jnibwa_createReferenceIndex.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
_lib.jnibwa_createIndexFile.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
_lib.jnibwa_openIndex.restype = ctypes.c_void_p
_lib.jnibwa_openIndex.argtypes = [ctypes.c_int]
_lib.jnibwa_destroyIndex.argtypes = [ctypes.c_void_p]
_lib.jnibwa_getRefContigNames.restype = ctypes.c_void_p
_lib.jnibwa_getRefContigNames.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
_lib.jnibwa_createAlignments.restype = ctypes.c_void_p
_lib.jnibwa_createAlignments.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
_lib.jnibwa_createDefaultOptions.restype = ctypes.c_void_p
_lib.jnibwa_free.argtypes = [ctypes.c_void_p]
_lib.jnibwa_getVersion.restype = ctypes.c_char_p
_lib.bwamem_hip_align_to_bam.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int]
_lib.bwamem_hip_align_to_bam_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p,
                                                ctypes.c_int, ctypes.c_int]
_lib.bwamem_hip_align_to_sorted_bam.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_int]
_vp, _sz, _i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64
_lib.bwamem_hip_batch_upload.restype = _vp; _lib.bwamem_hip_batch_upload.argtypes = [_vp, ctypes.c_char_p, _sz]
_lib.bwamem_hip_batch_free.restype = None; _lib.bwamem_hip_batch_free.argtypes = [_vp]
_lib.bwamem_hip_batch_keep_offsets.argtypes = [_vp, ctypes.c_int]
_lib.bwamem_hip_batch_align.argtypes = [_vp, _vp, _vp, _vp, _i64]
_lib.bwamem_hip_batch_set_qualities.argtypes = [_vp, ctypes.c_char_p, _sz]
_lib.bwamem_hip_batch_set_read_group.argtypes = [_vp, ctypes.c_char_p]
_lib.bwamem_hip_batch_encode_bam.argtypes = [_vp, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(_i64)]
_lib.bwamem_hip_batch_sort_bam.argtypes = [_vp]
_lib.bwamem_hip_batch_bam_bytes.restype = _sz; _lib.bwamem_hip_batch_bam_bytes.argtypes = [_vp]
_lib.bwamem_hip_batch_compress_bam.argtypes = [_vp, ctypes.c_int]
_lib.bwamem_hip_batch_bgzf_bytes.restype = _sz; _lib.bwamem_hip_batch_bgzf_bytes.argtypes = [_vp]
_lib.bwamem_hip_batch_bgzf_download.argtypes = [_vp, _vp]
_lib.bwamem_hip_batch_index_bam.restype = _vp; _lib.bwamem_hip_batch_index_bam.argtypes = [_vp, _i64, ctypes.POINTER(_sz)]
_lib.bwamem_hip_bam_header_rg.restype = _vp; _lib.bwamem_hip_bam_header_rg.argtypes = [_vp, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(_sz)]
_lib.bwamem_hip_bgzf_compress_device.restype = _vp; _lib.bwamem_hip_bgzf_compress_device.argtypes = [_vp, _vp, _sz, ctypes.c_int, ctypes.POINTER(_sz)]
_lib.bwamem_hip_align_fastq_to_bam.argtypes = [_vp, _vp, _vp, ctypes.c_char_p, _sz, ctypes.c_char_p, _sz, ctypes.c_char_p, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int]
_BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


class _DupCounts(ctypes.Structure):
    """bwamem_dup_counts_t"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("unpaired_reads_examined", "read_pairs_examined", "secondary_or_supplementary", "unmapped_reads",
                                               "unpaired_read_duplicates", "read_pair_duplicates")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


_lib.bwamem_hip_batch_mark_duplicates.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(_DupCounts)]
_lib.bwamem_hip_align_to_marked_bam.argtypes = [_vp, _vp, _vp, ctypes.c_char_p, _sz, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(_DupCounts)]
_lib.bwamem_hip_align_fastq_to_marked_bam.argtypes = [_vp, _vp, _vp, ctypes.c_char_p, _sz, ctypes.c_char_p, _sz, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_int, ctypes.c_int, ctypes.POINTER(_DupCounts)]
_lib.bwamem_hip_align_fastq_gz_to_marked_bam.argtypes = [_vp, _vp, _vp, ctypes.c_char_p, _sz, ctypes.c_char_p, _sz, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_DupCounts)]
_lib.bwamem_hip_bgzf_inflate_device.restype = _vp
_lib.bwamem_hip_bgzf_inflate_device.argtypes = [_vp, ctypes.c_char_p, _sz, ctypes.POINTER(_sz), ctypes.POINTER(ctypes.c_int64)]


class _BamOptions(ctypes.Structure):
    """bwamem_bam_options_t"""
    _fields_ = [("size", _sz), ("rg_line", ctypes.c_char_p), ("sort", ctypes.c_int), ("mark_dup", ctypes.c_int), ("tags", ctypes.c_uint),
                ("write_header", ctypes.c_int)]


_lib.bwamem_hip_batch_set_tags.argtypes = [_vp, ctypes.c_uint]
_lib.bwamem_hip_fastq_to_bam.argtypes = [_vp, _vp, _vp, ctypes.c_char_p, _sz, ctypes.c_char_p, _sz, ctypes.POINTER(_BamOptions), ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(_DupCounts)]
_TAG_BITS = {"SA": 1, "MC": 2, "MQ": 4}

_QC_PAIRS = ("total", "primary", "secondary", "supplementary", "duplicates", "primary_duplicates", "mapped", "primary_mapped", "paired", "read1", "read2",
             "properly_paired", "both_mapped", "singletons", "mate_diff_chr", "mate_diff_chr_mapq5")
_QC_SINGLES = ("unplaced", "sequences", "total_length", "max_length", "reads_mq0", "bases_mapped", "bases_mapped_cigar", "bases_soft_clipped", "ins_events",
               "ins_bases", "del_events", "del_bases", "mismatches", "records_without_nm")
_QC_ARRAYS = {"mapq_hist": 0, "qual_hist": 1, "isize_fr": 2, "isize_rf": 3, "isize_tandem": 4, "contig_mapped": 5, "contig_unmapped": 6}
_QC_REPORTS = {"flagstat": 0, "idxstats": 1, "summary": 2, "insert_size": 3}


class _QcCounts(ctypes.Structure):
    """bwamem_qc_counts_t"""
    _fields_ = ([(n, ctypes.c_uint64 * 2) for n in _QC_PAIRS] + [(n, ctypes.c_uint64) for n in _QC_SINGLES]
                + [("isize_min", ctypes.c_uint64 * 3), ("isize_max", ctypes.c_uint64 * 3)])


_lib.bwamem_hip_qc_create.restype = _vp; _lib.bwamem_hip_qc_create.argtypes = [_vp]
_lib.bwamem_hip_qc_free.restype = None; _lib.bwamem_hip_qc_free.argtypes = [_vp]
_lib.bwamem_hip_qc_add_batch.argtypes = [_vp, _vp]
_lib.bwamem_hip_qc_add_records_device.argtypes = [_vp, ctypes.c_char_p, _sz]
_lib.bwamem_hip_qc_counts.argtypes = [_vp, ctypes.POINTER(_QcCounts)]
_lib.bwamem_hip_qc_array.restype = _i64; _lib.bwamem_hip_qc_array.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), _sz]
_lib.bwamem_hip_qc_serialize.restype = _vp; _lib.bwamem_hip_qc_serialize.argtypes = [_vp, ctypes.POINTER(_sz)]
_lib.bwamem_hip_qc_add_serialized.argtypes = [_vp, ctypes.c_char_p, _sz]
_lib.bwamem_hip_qc_report.restype = _vp; _lib.bwamem_hip_qc_report.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(_sz)]
_lib.bwamem_hip_fastq_to_bam_qc.argtypes = [_vp, _vp, _vp, ctypes.c_char_p, _sz, ctypes.c_char_p, _sz, ctypes.POINTER(_BamOptions), ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(_DupCounts), _vp]

# base-level QC (csrc/bam_baseqc.h): the tables in the order of BWAMEM_HIP_BASEQC_*
_BASEQC_ARRAYS = {"base": 0, "qual_sum": 1, "qual_n": 2, "aligned": 3, "mism": 4, "ins": 5, "del_ev": 6, "soft": 7, "read_gc": 8, "gcb_reads": 9, "gcb_qual_sum": 10,
                  "gcb_qual_n": 11}
_BASEQC_REPORTS = {"cycles": 0, "gc": 1}


class _BaseQcCounts(ctypes.Structure):
    """bwamem_baseqc_counts_t"""
    _fields_ = [("records", ctypes.c_uint64 * 3), ("qcfail_skipped", ctypes.c_uint64), ("gcb_skipped", ctypes.c_uint64)]


_lib.bwamem_hip_baseqc_create.restype = _vp; _lib.bwamem_hip_baseqc_create.argtypes = [_vp]
_lib.bwamem_hip_baseqc_free.restype = None; _lib.bwamem_hip_baseqc_free.argtypes = [_vp]
_lib.bwamem_hip_baseqc_add_batch.argtypes = [_vp, _vp]
_lib.bwamem_hip_baseqc_add_records_device.argtypes = [_vp, ctypes.c_char_p, _sz]
_lib.bwamem_hip_baseqc_counts.argtypes = [_vp, ctypes.POINTER(_BaseQcCounts)]
_lib.bwamem_hip_baseqc_array.restype = _i64; _lib.bwamem_hip_baseqc_array.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), _sz]
_lib.bwamem_hip_baseqc_serialize.restype = _vp; _lib.bwamem_hip_baseqc_serialize.argtypes = [_vp, ctypes.POINTER(_sz)]
_lib.bwamem_hip_baseqc_add_serialized.argtypes = [_vp, ctypes.c_char_p, _sz]
_lib.bwamem_hip_baseqc_report.restype = _vp; _lib.bwamem_hip_baseqc_report.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(_sz)]
_lib.bwamem_hip_index_gc_windows.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint64)]
_lib.bwamem_hip_fastq_to_bam_metrics.argtypes = [_vp, _vp, _vp, ctypes.c_char_p, _sz, ctypes.c_char_p, _sz, ctypes.POINTER(_BamOptions), ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(_DupCounts), _vp, _vp]


def _tag_mask(tags):
    """("SA", "MC", "MQ") -> BWAMEM_HIP_TAG_* OR-ed"""
    if isinstance(tags, (str, bytes)):
        tags = (tags,)
    mask = 0
    for t in tags:
        t = t.decode() if isinstance(t, bytes) else t
        if t not in _TAG_BITS:
            raise ValueError("unknown tag %r: the optional tags are SA, MC and MQ" % (t,))
        mask |= _TAG_BITS[t]
    return mask


def _taken(p, n):
    out = ctypes.string_at(p, n)
    _lib.jnibwa_free(p)
    return out


class BwaMemQc:
    """Additive: an alignment-QC accumulator (csrc/bam_qc.h) -- flagstat, idxstats, summary numbers and insert sizes of the records
    of any number of alignSeqsToBam / alignFastqToBam calls (qc=...), reduced on the device while the records are there.  The index
    must stay open while batches are added."""

    def __init__(self, index):
        self.index = index
        self._q = _lib.bwamem_hip_qc_create(index.refIndex())
        index.deRefIndex()
        if not self._q:
            raise RuntimeError("Unable to create a QC accumulator for bwa-mem index %s" % index.indexImageFile)

    def _ptr(self):
        if not self._q:
            raise RuntimeError("The QC accumulator has been closed.")
        return self._q

    def close(self):
        if self._q:
            _lib.bwamem_hip_qc_free(self._q)
            self._q = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def counts(self):
        """every counter by its name; the flagstat counters as (QC-passed, QC-failed), isize_min / isize_max as (FR, RF, TANDEM)"""
        c = _QcCounts()
        if _lib.bwamem_hip_qc_counts(self._ptr(), ctypes.byref(c)) != 0:
            raise RuntimeError("bwamem_hip_qc_counts failed")
        out = {n: (int(getattr(c, n)[0]), int(getattr(c, n)[1])) for n in _QC_PAIRS}
        out.update({n: int(getattr(c, n)) for n in _QC_SINGLES})
        out["isize_min"], out["isize_max"] = tuple(int(x) for x in c.isize_min), tuple(int(x) for x in c.isize_max)
        return out

    def array(self, name):
        """mapq_hist, qual_hist, isize_fr, isize_rf, isize_tandem, contig_mapped or contig_unmapped, as a list of ints"""
        if name not in _QC_ARRAYS:
            raise ValueError("unknown QC array %r: %s" % (name, ", ".join(sorted(_QC_ARRAYS))))
        n = _lib.bwamem_hip_qc_array(self._ptr(), _QC_ARRAYS[name], None, 0)
        buf = (ctypes.c_uint64 * max(n, 1))()
        _lib.bwamem_hip_qc_array(self._ptr(), _QC_ARRAYS[name], buf, n)
        return [int(x) for x in buf[:n]]

    def _report(self, kind):
        sz = ctypes.c_size_t()
        p = _lib.bwamem_hip_qc_report(self._ptr(), _QC_REPORTS[kind], ctypes.byref(sz))
        if not p:
            raise RuntimeError("bwamem_hip_qc_report failed")
        return _taken(p, sz.value).decode()

    def flagstat(self): return self._report("flagstat")
    def idxstats(self): return self._report("idxstats")
    def summary(self): return self._report("summary")
    def insertSizeMetrics(self): return self._report("insert_size")

    def serialize(self):
        sz = ctypes.c_size_t()
        p = _lib.bwamem_hip_qc_serialize(self._ptr(), ctypes.byref(sz))
        if not p:
            raise RuntimeError("bwamem_hip_qc_serialize failed")
        return _taken(p, sz.value)

    def add(self, other):
        """adds another accumulator, or the bytes of one (serialize(): other calls, devices, ranks); ValueError when it is of another index"""
        blob = other.serialize() if isinstance(other, BwaMemQc) else bytes(other)
        if _lib.bwamem_hip_qc_add_serialized(self._ptr(), blob, len(blob)) != 0:
            raise ValueError("the QC blob was refused: another version, or an index with another number of contigs")


class BwaMemBaseQc:
    """Additive: a base-level QC accumulator (csrc/bam_baseqc.h) -- quality, base composition, mismatches, indels and soft clips per
    sequencing cycle and end, the reads' GC histograms and GC bias over 100-base reference windows -- of the records of any number of
    alignSeqsToBam / alignFastqToBam calls (base_qc=...), reduced on the device against the resident reference.  The index must stay
    open while batches are added.  serialize() / add() have the shape of BwaMemQc's, so sharding.gather_qc carries this accumulator
    unchanged."""

    def __init__(self, index):
        self.index = index
        self._q = _lib.bwamem_hip_baseqc_create(index.refIndex())
        index.deRefIndex()
        if not self._q:
            raise RuntimeError("Unable to create a base-QC accumulator for bwa-mem index %s" % index.indexImageFile)

    def _ptr(self):
        if not self._q:
            raise RuntimeError("The base-QC accumulator has been closed.")
        return self._q

    def close(self):
        if self._q:
            _lib.bwamem_hip_baseqc_free(self._q)
            self._q = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def counts(self):
        """records (one count per end: unpaired, first, second), qcfail_skipped, gcb_skipped"""
        c = _BaseQcCounts()
        if _lib.bwamem_hip_baseqc_counts(self._ptr(), ctypes.byref(c)) != 0:
            raise RuntimeError("bwamem_hip_baseqc_counts failed")
        return dict(records=[int(x) for x in c.records], qcfail_skipped=int(c.qcfail_skipped), gcb_skipped=int(c.gcb_skipped))

    def array(self, name):
        """one table as a flat list of ints.  qual_sum, qual_n, aligned, mism, ins, del_ev, soft: [end][cycle], 3 x 1024; base:
        [end][cycle][A C G T N]; read_gc: [end][101]; gcb_reads, gcb_qual_sum, gcb_qual_n: [101]"""
        if name not in _BASEQC_ARRAYS:
            raise ValueError("unknown base-QC table %r: %s" % (name, ", ".join(sorted(_BASEQC_ARRAYS))))
        n = _lib.bwamem_hip_baseqc_array(self._ptr(), _BASEQC_ARRAYS[name], None, 0)
        buf = (ctypes.c_uint64 * max(n, 1))()
        _lib.bwamem_hip_baseqc_array(self._ptr(), _BASEQC_ARRAYS[name], buf, n)
        return [int(x) for x in buf[:n]]

    def _report(self, kind):
        sz = ctypes.c_size_t()
        p = _lib.bwamem_hip_baseqc_report(self._ptr(), _BASEQC_REPORTS[kind], ctypes.byref(sz))
        if not p:
            raise RuntimeError("bwamem_hip_baseqc_report failed")
        return _taken(p, sz.value).decode()

    def cycles(self): return self._report("cycles")
    def gcBias(self): return self._report("gc")

    def serialize(self):
        sz = ctypes.c_size_t()
        p = _lib.bwamem_hip_baseqc_serialize(self._ptr(), ctypes.byref(sz))
        if not p:
            raise RuntimeError("bwamem_hip_baseqc_serialize failed")
        return _taken(p, sz.value)

    def add(self, other):
        """adds another accumulator, or the bytes of one (serialize(): other calls, devices, ranks); ValueError when it is refused"""
        blob = other.serialize() if isinstance(other, BwaMemBaseQc) else bytes(other)
        if _lib.bwamem_hip_baseqc_add_serialized(self._ptr(), blob, len(blob)) != 0:
            raise ValueError("the base-QC blob was refused: another type or version, or an index with another number of contigs")


class CouldNotReadImageException(RuntimeError):
    pass


class CouldNotCreateIndexException(RuntimeError):
    pass


class BwaMemPairEndStats:
    DEFAULT_LOW_AND_HIGH_SIGMA = 4
    DEFAULT_STD_TO_AVERAGE_RATIO = .1

    def __init__(self, average=None, std=None, low=None, high=None, _failed=False):
        if _failed:
            self.failed, self.average, self.std, self.low, self.high = True, float("nan"), float("nan"), 0, 0
            return
        if std is None:
            std = average * self.DEFAULT_STD_TO_AVERAGE_RATIO
        if low is None:
            low = max(1, int(math.floor(average - self.DEFAULT_LOW_AND_HIGH_SIGMA * std + 0.5)))
            high = max(1, int(math.floor(average + self.DEFAULT_LOW_AND_HIGH_SIGMA * std + 0.5)))
        if math.isnan(average) or math.isinf(average) or average < 1:
            raise ValueError("invalid input average: %r" % average)
        if math.isnan(std) or math.isinf(std) or std < 0:
            raise ValueError("invalid std. err: %r" % std)
        if low > average:
            raise ValueError("the low limit cannot be larger than the average")
        if high < average:
            raise ValueError("the high limit cannot be larger than the average")
        self.failed, self.average, self.std, self.low, self.high = False, float(average), float(std), int(low), int(high)

    def _pack(self):
        """mem_pestat_t[4] as ...BwaMemIndex.c:21-40 fills it: slot 1 (FR) from this object, the rest failed."""
        b = b""
        for i in range(4):
            if i == 1 and not self.failed:
                b += struct.pack("<iiiidd", self.low, self.high, 0, 0, self.average, self.std)
            else:
                b += struct.pack("<iiiidd", 0, 0, 1, 0, 0.0, 0.0)
        return b


BwaMemPairEndStats.FAILED = BwaMemPairEndStats(_failed=True)
BwaMemPairEndStats.DO_NOT_INFER = BwaMemPairEndStats.FAILED


class BwaMemAlignment:
    def __init__(self, samFlag, refId, refStart, refEnd, seqStart, seqEnd, mapQual, nMismatches, alignerScore,
                 suboptimalScore, cigar, mdTag, xaTag, mateRefId, mateRefStart, templateLen):
        self.samFlag, self.refId, self.refStart, self.refEnd = samFlag, refId, refStart, refEnd
        self.seqStart, self.seqEnd, self.mapQual, self.nMismatches = seqStart, seqEnd, mapQual, nMismatches
        self.alignerScore, self.suboptimalScore, self.cigar, self.mdTag, self.xaTag = alignerScore, suboptimalScore, cigar, mdTag, xaTag
        self.mateRefId, self.mateRefStart, self.templateLen = mateRefId, mateRefStart, templateLen

    def getSamFlag(self): return self.samFlag
    def getRefId(self): return self.refId
    def getRefStart(self): return self.refStart
    def getRefEnd(self): return self.refEnd
    def getSeqStart(self): return self.seqStart
    def getSeqEnd(self): return self.seqEnd
    def getMapQual(self): return self.mapQual
    def getNMismatches(self): return self.nMismatches
    def getAlignerScore(self): return self.alignerScore
    def getSuboptimalScore(self): return self.suboptimalScore
    def getCigar(self): return self.cigar
    def getMDTag(self): return self.mdTag
    def getXATag(self): return self.xaTag
    def getMateRefId(self): return self.mateRefId
    def getMateRefStart(self): return self.mateRefStart
    def getTemplateLen(self): return self.templateLen


class BwaMemIndex:
    INDEX_FILE_EXTENSIONS = [".amb", ".ann", ".bwt", ".pac", ".sa"]
    IMAGE_FILE_EXTENSION = ".img"
    _class_lock = threading.Lock()

    @staticmethod
    def createIndexImageFromIndexFiles(indexPrefix, imageFile):
        if indexPrefix is None:
            raise ValueError("the index prefix cannot be null")
        if imageFile is None:
            raise ValueError("the image file cannot be null")
        for ext in BwaMemIndex.INDEX_FILE_EXTENSIONS:       # assertLooksLikeIndexPrefix, BwaMemIndex.java:259-266
            fn = indexPrefix + ext
            if not (os.path.isfile(fn) and os.path.getsize(fn) > 0):
                raise ValueError("index file %s is missing or empty" % fn)
        _lib.jnibwa_createIndexFile(indexPrefix.encode(), imageFile.encode())   # result discarded, BwaMemIndex.java:122

    @staticmethod
    def createIndexImageFromFastaFile(fasta, imageFile=None, algo="auto"):
        if imageFile is None:
            imageFile = fasta + BwaMemIndex.IMAGE_FILE_EXTENSION
        if not (os.path.isfile(fasta) and os.path.getsize(fasta) > 0):
            raise ValueError("the fasta file %s is missing or empty" % fasta)
        import tempfile
        tmp = tempfile.mkdtemp()
        prefix = os.path.join(tmp, os.path.basename(fasta))
        try:
            rc = _lib.jnibwa_createReferenceIndex(fasta.encode(), prefix.encode(), algo.encode())
            if rc == -1:
                raise ValueError("wrong algorithm name '%s'" % algo)     # ...BwaMemIndex.c:52-58
            _lib.jnibwa_createIndexFile(prefix.encode(), imageFile.encode())
        finally:
            for ext in BwaMemIndex.INDEX_FILE_EXTENSIONS:
                try:
                    os.unlink(prefix + ext)
                except OSError:
                    pass
            os.rmdir(tmp)
        return imageFile

    def __init__(self, indexImageFile):
        self.indexImageFile = indexImageFile
        if not (os.path.isfile(indexImageFile) and os.path.getsize(indexImageFile) > 0):
            raise CouldNotReadImageException("%s is empty or is not readable" % indexImageFile)
        self._refCount = 0
        self._lock = threading.Lock()
        fd = os.open(indexImageFile, os.O_RDONLY)          # ...BwaMemIndex.c:74-81
        self.indexAddress = _lib.jnibwa_openIndex(fd) or 0
        if not self.indexAddress:
            raise CouldNotReadImageException("%s: unable to open bwa-mem index" % indexImageFile)
        sz = ctypes.c_size_t()
        p = _lib.jnibwa_getRefContigNames(self.indexAddress, ctypes.byref(sz))
        if not p:
            raise CouldNotReadImageException("unable to retrieve reference contig names from bwa-mem index")
        buf = ctypes.string_at(p, sz.value)
        _lib.jnibwa_free(p)
        n, = struct.unpack_from("=i", buf, 0)
        off, self.refContigNames = 4, []
        for _ in range(n):
            l, = struct.unpack_from("=i", buf, off); off += 4
            self.refContigNames.append(buf[off:off + l].decode()); off += l

    def isOpen(self):
        return self.indexAddress != 0

    def refIndex(self):
        with self._lock:
            self._refCount += 1
        if not self.indexAddress:
            raise RuntimeError("Index image %s has been closed" % self.indexImageFile)
        return self.indexAddress

    def deRefIndex(self):
        with self._lock:
            self._refCount -= 1

    def close(self):
        if self.indexAddress:
            with BwaMemIndex._class_lock:
                if self.indexAddress:
                    if self._refCount != 0:
                        raise RuntimeError("Index image %s can't be closed:  it's in use." % self.indexImageFile)
                    addr, self.indexAddress = self.indexAddress, 0
                    _lib.jnibwa_destroyIndex(addr)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def getReferenceContigNames(self):
        return self.refContigNames

    def gcWindows(self):
        """Additive: windows[g], g = 0..100 -- the number of 100-base windows of the reference that touch no .amb hole and hold g C/G
        bases: the denominator of GC bias (csrc/bam_baseqc.h), computed on the device once per index"""
        out = (ctypes.c_uint64 * 101)()
        idx = self.refIndex()
        try:
            if _lib.bwamem_hip_index_gc_windows(idx, out) != 0:
                raise RuntimeError("bwamem_hip_index_gc_windows failed for bwa-mem index %s" % self.indexImageFile)
        finally:
            self.deRefIndex()
        return [int(x) for x in out]

    @staticmethod
    def getBWAVersion():
        return _lib.jnibwa_getVersion().decode()

    def doAlignment(self, seqs, opts, peStats):
        sz = ctypes.c_size_t()
        pb = ctypes.create_string_buffer(peStats._pack(), 128) if peStats is not None else None
        p = _lib.jnibwa_createAlignments(self.indexAddress, opts, pb, seqs, ctypes.byref(sz))
        if not p:
            raise RuntimeError("Unable to get alignments from bwa-mem index %s: We don't know why." % self.indexImageFile)
        out = ctypes.string_at(p, sz.value)
        _lib.jnibwa_free(p)
        return out


def _opt_int(off):
    return (lambda self: struct.unpack_from("=i", self._getOpts(), off)[0],
            lambda self, v: struct.pack_into("=i", self._getOpts(), off, v))


def _opt_float(off):
    return (lambda self: struct.unpack_from("=f", self._getOpts(), off)[0],
            lambda self, v: struct.pack_into("=f", self._getOpts(), off, v))


class BwaMemAligner:
    MEM_F_PE, MEM_F_NOPAIRING, MEM_F_ALL, MEM_F_NO_MULTI, MEM_F_NO_RESCUE = 0x2, 0x4, 0x8, 0x10, 0x20
    MEM_F_REF_HDR, MEM_F_SOFTCLIP, MEM_F_SMARTPE, MEM_F_PRIMARY5 = 0x100, 0x200, 0x400, 0x800

    def __init__(self, index):
        self.index = index
        if not index.isOpen():
            raise RuntimeError("Can't create aligner: bwa-mem index has been closed")
        p = _lib.jnibwa_createDefaultOptions()
        self.opts = (ctypes.c_char * 168).from_buffer_copy(ctypes.string_at(p, 168))
        _lib.jnibwa_free(p)
        self.pairEndStats = None

    def isOpen(self):
        return self.opts is not None

    def close(self):
        self.opts = None

    def _getOpts(self):
        if self.opts is None:
            raise RuntimeError("The aligner has been closed.")
        return self.opts

    # option accessors by byte offset, BwaMemAligner.java:46-136
    getMatchScoreOption, setMatchScoreOption = _opt_int(0)
    getMismatchPenaltyOption, setMismatchPenaltyOption = _opt_int(4)
    getDGapOpenPenaltyOption, setDGapOpenPenaltyOption = _opt_int(8)
    getDGapExtendPenaltyOption, setDGapExtendPenaltyOption = _opt_int(12)
    getIGapOpenPenaltyOption, setIGapOpenPenaltyOption = _opt_int(16)
    getIGapExtendPenaltyOption, setIGapExtendPenaltyOption = _opt_int(20)
    getUnpairedPenaltyOption, setUnpairedPenaltyOption = _opt_int(24)
    getClip5PenaltyOption, setClip5PenaltyOption = _opt_int(28)
    getClip3PenaltyOption, setClip3PenaltyOption = _opt_int(32)
    getBandwidthOption, setBandwidthOption = _opt_int(36)
    getZDropOption, setZDropOption = _opt_int(40)
    getOutputScoreThresholdOption, setOutputScoreThresholdOption = _opt_int(56)
    getFlagOption, setFlagOption = _opt_int(60)
    getMinSeedLengthOption, setMinSeedLengthOption = _opt_int(64)
    getMinChainWeightOption, setMinChainWeightOption = _opt_int(68)
    getMaxChainExtendOption, setMaxChainExtendOption = _opt_int(72)
    getSplitFactorOption, setSplitFactorOption = _opt_float(76)
    getSplitWidthOption, setSplitWidthOption = _opt_int(80)
    getMaxSeedOccurencesOption, setMaxSeedOccurencesOption = _opt_int(84)
    getMaxChainGapOption, setMaxChainGapOption = _opt_int(88)
    getNThreadsOption, setNThreadsOption = _opt_int(92)
    getChunkSizeOption, setChunkSizeOption = _opt_int(96)
    getMaskLevelOption, setMaxLevelOption = _opt_float(100)
    getDropRatioOption, setDropRatioOption = _opt_float(104)
    getXADropRatio, setXADropRatio = _opt_float(108)
    getMaskLevelRedunOption, setMaskLevelRedunOption = _opt_float(112)
    getMapQCoefLenOption, setMapQCoefLenOption = _opt_float(116)
    getMapQCoefFacOption, setMapQCoefFacOption = _opt_int(120)
    getMaxInsOption, setMaxInsOption = _opt_int(124)
    getMaxMateSWOption, setMaxMateSWOption = _opt_int(128)
    getMaxXAHitsOption, setMaxXAHitsOption = _opt_int(132)
    getMaxXAHitsAltOption, setMaxXAHitsAltOption = _opt_int(136)

    def getMaxMemIntvOption(self): return struct.unpack_from("=q", self._getOpts(), 48)[0]
    def setMaxMemIntvOption(self, v): struct.pack_into("=q", self._getOpts(), 48, v)
    def getScoringMatrixOption(self): return bytes(self._getOpts()[140:165])
    def setScoringMatrixOption(self, mat): self._getOpts()[140:165] = bytes(x & 0xff for x in mat)
    def getExpectedOptsSize(self): return 168
    def getOptsSize(self): return len(self._getOpts())

    def alignPairs(self): self.setFlagOption(self.MEM_F_PE | self.getFlagOption())

    def setIntraCtgOptions(self):
        self.setDGapOpenPenaltyOption(16); self.setIGapOpenPenaltyOption(16); self.setMismatchPenaltyOption(9)
        self.setClip5PenaltyOption(5); self.setClip3PenaltyOption(5)

    def inferPairEndStats(self): self.pairEndStats = None
    def dontInferPairEndStats(self): self.pairEndStats = BwaMemPairEndStats.DO_NOT_INFER
    def setProperPairEndStats(self, stats): self.pairEndStats = stats
    def getIndex(self): return self.index

    def newQc(self):
        """Additive: an empty QC accumulator (BwaMemQc) for this aligner's index, to be handed to alignSeqsToBam / alignFastqToBam"""
        return BwaMemQc(self.index)

    def newBaseQc(self):
        """Additive: an empty base-level QC accumulator (BwaMemBaseQc) for this aligner's index, to be handed to alignSeqsToBam /
        alignFastqToBam as base_qc="""
        return BwaMemBaseQc(self.index)

    def alignSeqsRaw(self, sequences, func=lambda s: s):
        """the raw native response (BwaMemAligner.java:192-214)"""
        opts = self._getOpts()
        self.index.refIndex()
        try:
            seqs = [func(e) for e in sequences]
            seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
            buf = struct.pack("=i", len(seqs)) + b"".join(s + b"\0" for s in seqs)
            contigBuf = ctypes.create_string_buffer(buf, len(buf))
            self._n = len(seqs)
            return self.index.doAlignment(contigBuf, opts, self.pairEndStats)
        finally:
            self.index.deRefIndex()

    def alignSeqsToBam(self, sequences, path, names=None, level=1, func=lambda s: s, device=False, sort=False, index_path=None, quals=None,
                       read_group=None, mark_duplicates=False, tags=(), qc=None, base_qc=None):
        """Additive (no Java counterpart): align and write a BAM file -- header, the records encoded on the device, BGZF framing at
        `level` (0 = stored blocks; 1..9 need libz.so.1), EOF block.  names: one per sequence (1..254 bytes each), else
        "r<index>" / "p<pair index>".  The insert-size statistics are the aligner's (setProperPairEndStats / inferred).
        device=True: the BGZF blocks are compressed on the device as well (DEFLATE with dynamic Huffman codes; `level` is ignored
        and libz is not needed).
        sort=True (implies device=True): the records are coordinate-sorted on the device within this call and the header says
        SO:coordinate; index_path: the BAI index of that file is written there as well (needs sort=True).
        quals: one Phred+33 string per sequence, each as long as its sequence: the records carry them as QUAL.  read_group: an
        "@RG\\tID:..." header line: it goes into the header, and every record carries RG:Z:<ID>.  Either implies device=True.
        mark_duplicates=True (needs device=True, sort=True, quals or read_group: the records have to stay on the device): duplicates
        are marked on the device within this call before the sort (csrc/bam_dup.h), and the counts are returned as a dict.
        tags: any of "SA", "MC", "MQ": the records carry them, built on the device (csrc/bam_encode.h); implies device=True.
        qc: a BwaMemQc (newQc()): the records of this call are added to it on the device, after the marking and before the sort, once
        the call has succeeded (csrc/bam_qc.h); accepted where mark_duplicates is.
        base_qc: a BwaMemBaseQc (newBaseQc()): the same for the base-level tables (csrc/bam_baseqc.h)."""
        mask = _tag_mask(tags)
        if index_path is not None and not sort:
            raise ValueError("index_path needs sort=True: only a coordinate-sorted file has a BAI index")
        if (mark_duplicates or qc is not None or base_qc is not None) and not (device or sort or quals is not None or read_group is not None or mask):
            raise ValueError("mark_duplicates, qc and base_qc need device=True or sort=True: the host-framing path takes the records off the device unmarked")
        opts = self._getOpts()
        seqs = [func(e) for e in sequences]
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        if names is not None and len(names) != len(seqs):
            raise ValueError("%d names for %d sequences" % (len(names), len(seqs)))
        if quals is not None or read_group is not None or mask or qc is not None or base_qc is not None:
            return self._alignSeqsToBamBatch(seqs, path, names, sort, index_path, quals, read_group, mark_duplicates, mask, qc, base_qc)
        buf = struct.pack("=i", len(seqs)) + b"".join(s + b"\0" for s in seqs)
        arr = None
        if names is not None:
            arr = (ctypes.c_char_p * len(names))(*[n.encode() if isinstance(n, str) else bytes(n) for n in names])
        pes = self.pairEndStats
        pb = ctypes.create_string_buffer(pes._pack(), 128) if pes is not None else None
        counts = _DupCounts()
        self.index.refIndex()
        try:
            fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            try:
                if mark_duplicates:
                    fd_bai = os.open(index_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) if index_path is not None else -1
                    try:
                        rc = _lib.bwamem_hip_align_to_marked_bam(self.index.indexAddress, opts, pb, buf, len(buf), arr, 1 if sort else 0, fd, fd_bai, 1,
                                                                 ctypes.byref(counts))
                    finally:
                        if fd_bai >= 0:
                            os.close(fd_bai)
                elif sort:
                    fd_bai = os.open(index_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) if index_path is not None else -1
                    try:
                        rc = _lib.bwamem_hip_align_to_sorted_bam(self.index.indexAddress, opts, pb, buf, len(buf), arr, fd, fd_bai, 1)
                    finally:
                        if fd_bai >= 0:
                            os.close(fd_bai)
                elif device:
                    rc = _lib.bwamem_hip_align_to_bam_device(self.index.indexAddress, opts, pb, buf, len(buf), arr, fd, 1)
                else:
                    rc = _lib.bwamem_hip_align_to_bam(self.index.indexAddress, opts, pb, buf, len(buf), arr, level, fd, 1)
            finally:
                os.close(fd)
        finally:
            self.index.deRefIndex()
        if rc != 0:
            raise RuntimeError("Unable to write alignments of bwa-mem index %s to %s" % (self.index.indexImageFile, path))
        return counts.as_dict() if mark_duplicates else None

    def _alignSeqsToBamBatch(self, seqs, path, names, sort, index_path, quals, read_group, mark_duplicates=False, tag_mask=0, qc=None, base_qc=None):
        """alignSeqsToBam through the batch calls, which take qualities and a read group; nothing is written unless all of it succeeds"""
        if quals is not None:
            quals = [q.encode() if isinstance(q, str) else bytes(q) for q in quals]
            if len(quals) != len(seqs) or any(len(q) != len(s) for q, s in zip(quals, seqs)):
                raise ValueError("one quality string per sequence, each as long as its sequence")
        rg = None if read_group is None else read_group.encode() if isinstance(read_group, str) else bytes(read_group)
        buf = struct.pack("=i", len(seqs)) + b"".join(s + b"\0" for s in seqs)
        blob, off = None, None
        if names is not None:
            enc = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
            ends = [0]
            for n in enc:
                ends.append(ends[-1] + len(n))
            blob, off = b"".join(enc), (ctypes.c_int64 * len(ends))(*ends)
        pes = self.pairEndStats
        pb = ctypes.create_string_buffer(pes._pack(), 128) if pes is not None else None
        paired = 1 if self.getFlagOption() & self.MEM_F_PE else 0
        fail = RuntimeError("Unable to write alignments of bwa-mem index %s to %s" % (self.index.indexImageFile, path))
        idx = self.index.refIndex()
        b = None
        try:
            b = _lib.bwamem_hip_batch_upload(idx, buf, len(buf))
            if not b:
                raise fail
            if quals is not None:
                qb = b"".join(q + b"\0" for q in quals)
                if _lib.bwamem_hip_batch_set_qualities(b, qb, len(qb)) != 0:
                    raise ValueError("the qualities were refused: every byte must be in 33..126")
            if rg is not None and _lib.bwamem_hip_batch_set_read_group(b, rg) != 0:
                raise ValueError("the read group was refused: one '@RG\\t' line with an ID: field of 1..254 bytes")
            if tag_mask and _lib.bwamem_hip_batch_set_tags(b, tag_mask) != 0:
                raise fail
            if _lib.bwamem_hip_batch_keep_offsets(b, 1) != 0 or _lib.bwamem_hip_batch_align(idx, self._getOpts(), pb, b, 0) != 0:
                raise fail
            counts = _DupCounts()
            if _lib.bwamem_hip_batch_encode_bam(b, paired, blob, off) != 0:
                raise fail
            if mark_duplicates and _lib.bwamem_hip_batch_mark_duplicates(b, paired, ctypes.byref(counts)) != 0:
                raise fail
            if qc is not None:                                          # into an accumulator of its own: qc takes it when the files are written
                qc._ptr()
                mine = BwaMemQc(self.index)
                if _lib.bwamem_hip_qc_add_batch(mine._ptr(), b) != 0:
                    raise fail
                qc_blob = mine.serialize()
                mine.close()
            if base_qc is not None:
                base_qc._ptr()
                mine = BwaMemBaseQc(self.index)
                if _lib.bwamem_hip_baseqc_add_batch(mine._ptr(), b) != 0:
                    raise fail
                base_blob = mine.serialize()
                mine.close()
            if sort and _lib.bwamem_hip_batch_sort_bam(b) != 0:
                raise fail
            sz = ctypes.c_size_t()
            p = _lib.bwamem_hip_bam_header_rg(idx, 1 if sort else 0, rg, ctypes.byref(sz))
            if not p:
                raise fail
            hdr = _taken(p, sz.value)
            p = _lib.bwamem_hip_bgzf_compress_device(idx, hdr, len(hdr), 0, ctypes.byref(sz))
            if not p:
                raise fail
            zh, z, bai = _taken(p, sz.value), _BGZF_EOF, None
            if _lib.bwamem_hip_batch_bam_bytes(b):
                if _lib.bwamem_hip_batch_compress_bam(b, 1) != 0:
                    raise fail
                zb = ctypes.create_string_buffer(_lib.bwamem_hip_batch_bgzf_bytes(b))
                if _lib.bwamem_hip_batch_bgzf_download(b, zb) != 0:
                    raise fail
                z = zb.raw
            if index_path is not None:
                p = _lib.bwamem_hip_batch_index_bam(b, len(zh), ctypes.byref(sz))
                if not p:
                    raise fail
                bai = _taken(p, sz.value)
        finally:
            if b:
                _lib.bwamem_hip_batch_free(b)
            self.index.deRefIndex()
        with open(path, "wb") as f:
            f.write(zh + z)
        if bai is not None:
            with open(index_path, "wb") as f:
                f.write(bai)
        if qc is not None:
            qc.add(qc_blob)
        if base_qc is not None:
            base_qc.add(base_blob)
        return counts.as_dict() if mark_duplicates else None

    def alignFastqToBam(self, fastq1, path, fastq2=None, read_group=None, sort=False, index_path=None, mark_duplicates=False, tags=(), qc=None, base_qc=None):
        """Additive: FASTQ in, a BAM file out.  fastq1 / fastq2: FASTQ text (bytes), or the path of a FASTQ file (str); bytes or a
        file that begin with 1f 8b are compressed FASTQ and are handed over as they are: BGZF (bgzip) is inflated on the device, plain
        gzip on the host (csrc/bgzf_inflate.h);
        with fastq2 the two hold the first and second reads of the pairs, without it fastq1 holds single-end reads or -- after
        alignPairs() -- interleaved pairs.  The text is taken apart on the device: the records carry the reads' names and base
        qualities, and RG:Z:<ID> when read_group (an "@RG\\tID:..." header line) is given.  sort / index_path as alignSeqsToBam.
        mark_duplicates=True: duplicates are marked on the device within this call, before the sort (csrc/bam_dup.h -- the highest
        sum of base qualities keeps a group's place), and the counts are returned as a dict.
        tags: any of "SA", "MC", "MQ", as for alignSeqsToBam; the call then goes through bwamem_hip_fastq_to_bam.
        qc: a BwaMemQc, as for alignSeqsToBam; the call then goes through bwamem_hip_fastq_to_bam_qc.
        base_qc: a BwaMemBaseQc, as for alignSeqsToBam; the call then goes through bwamem_hip_fastq_to_bam_metrics."""
        mask = _tag_mask(tags)
        if index_path is not None and not sort:
            raise ValueError("index_path needs sort=True: only a coordinate-sorted file has a BAI index")
        opts = self._getOpts()

        def text(x):
            if x is None or isinstance(x, (bytes, bytearray)):
                return None if x is None else bytes(x)
            with open(x, "rb") as f:
                return f.read()
        t1, t2 = text(fastq1), text(fastq2)
        rg = None if read_group is None else read_group.encode() if isinstance(read_group, str) else bytes(read_group)
        pes = self.pairEndStats
        pb = ctypes.create_string_buffer(pes._pack(), 128) if pes is not None else None
        counts = _DupCounts()
        idx = self.index.refIndex()
        try:
            fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            fd_bai = os.open(index_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) if index_path is not None else -1
            try:
                if base_qc is not None:
                    o = _BamOptions(size=ctypes.sizeof(_BamOptions), rg_line=rg, sort=1 if sort else 0, mark_dup=1 if mark_duplicates else 0, tags=mask, write_header=1)
                    rc = _lib.bwamem_hip_fastq_to_bam_metrics(idx, opts, pb, t1, len(t1), t2, len(t2) if t2 is not None else 0, ctypes.byref(o), fd, fd_bai,
                                                              ctypes.byref(counts), qc._ptr() if qc is not None else None, base_qc._ptr())
                elif mask or qc is not None:
                    o = _BamOptions(size=ctypes.sizeof(_BamOptions), rg_line=rg, sort=1 if sort else 0, mark_dup=1 if mark_duplicates else 0, tags=mask, write_header=1)
                    rc = _lib.bwamem_hip_fastq_to_bam_qc(idx, opts, pb, t1, len(t1), t2, len(t2) if t2 is not None else 0, ctypes.byref(o), fd, fd_bai, ctypes.byref(counts),
                                                         qc._ptr() if qc is not None else None)
                elif any(t is not None and t[:2] == b"\x1f\x8b" for t in (t1, t2)):
                    if not all(t is None or t[:2] == b"\x1f\x8b" for t in (t1, t2)):
                        raise ValueError("fastq1 and fastq2 must both be compressed or both be text")
                    rc = _lib.bwamem_hip_align_fastq_gz_to_marked_bam(idx, opts, pb, t1, len(t1), t2, len(t2) if t2 is not None else 0, rg, 1 if sort else 0, fd, fd_bai, 1,
                                                                      1 if mark_duplicates else 0, ctypes.byref(counts))
                elif mark_duplicates:
                    rc = _lib.bwamem_hip_align_fastq_to_marked_bam(idx, opts, pb, t1, len(t1), t2, len(t2) if t2 is not None else 0, rg, 1 if sort else 0, fd, fd_bai, 1,
                                                                   ctypes.byref(counts))
                else:
                    rc = _lib.bwamem_hip_align_fastq_to_bam(idx, opts, pb, t1, len(t1), t2, len(t2) if t2 is not None else 0, rg, 1 if sort else 0, fd, fd_bai, 1)
            finally:
                os.close(fd)
                if fd_bai >= 0:
                    os.close(fd_bai)
        finally:
            self.index.deRefIndex()
        if rc != 0:
            raise RuntimeError("Unable to write alignments of bwa-mem index %s to %s (malformed FASTQ, or a device error)" % (self.index.indexImageFile, path))
        return counts.as_dict() if mark_duplicates else None

    def inflateBgzf(self, data):
        """Additive, for tooling: the bytes of a BGZF stream inflated on the device (the counterpart of the device compressor).  Raises
        ValueError naming the smallest member that does not inflate."""
        data = bytes(data)
        sz, bad = ctypes.c_size_t(), ctypes.c_int64(-1)
        idx = self.index.refIndex()
        try:
            p = _lib.bwamem_hip_bgzf_inflate_device(idx, data, len(data), ctypes.byref(sz), ctypes.byref(bad))
        finally:
            self.index.deRefIndex()
        if not p:
            raise ValueError("not a BGZF stream that inflates (member %d)" % bad.value)
        try:
            return ctypes.string_at(p, sz.value)
        finally:
            _lib.jnibwa_free(p)

    def alignSeqs(self, sequences, func=lambda s: s):
        """BwaMemAligner.java:192-310: one list of BwaMemAlignment per input sequence"""
        buf = self.alignSeqsRaw(sequences, func)
        nSequences, off, out = self._n, 0, []
        ops = "MID?S???????????"
        for _ in range(nSequences):
            nAligns, = struct.unpack_from("=i", buf, off); off += 4
            alignments = []
            for _ in range(nAligns):
                flag_mapQ, = struct.unpack_from("=i", buf, off); off += 4
                flags, mapQual = (flag_mapQ >> 16) & 0xffff, flag_mapQ & 0xff
                if flags & 0x4:
                    refId = refStart = refEnd = seqStart = seqEnd = -1
                    nMismatches = alignerScore = suboptimalScore = 0
                    cigar, mdTag, xaTag = "", None, None
                else:
                    refId, refStart, nMismatches, alignerScore, suboptimalScore, nCigarOps = struct.unpack_from("=6i", buf, off); off += 24
                    cigar, refLen, seqLen, seqStart = "", 0, 0, 0
                    for i in range(max(nCigarOps, 0)):
                        lenOp, = struct.unpack_from("=I", buf, off); off += 4
                        ln, op = lenOp >> 4, ops[lenOp & 0xf]
                        cigar += "%d%s" % (ln, op)
                        if i == 0 and op == "S": seqStart = ln
                        if op in "MD": refLen += ln
                        if op in "MI": seqLen += ln
                    refEnd, seqEnd = refStart + refLen, seqStart + seqLen
                    tags = []
                    for _t in range(2):
                        tagLen, = struct.unpack_from("=i", buf, off); off += 4
                        tags.append(buf[off:off + tagLen].decode() if tagLen else None)
                        off += (tagLen + 3) & ~3
                    mdTag, xaTag = tags
                if (flags & 0x1) == 0 or (flags & 0x8) != 0:
                    mateRefId, mateStartPos, templateLen = -1, -1, 0
                else:
                    mateRefId, mateStartPos, templateLen = struct.unpack_from("=3i", buf, off); off += 12
                alignments.append(BwaMemAlignment(flags, refId, refStart, refEnd, seqStart, seqEnd, mapQual, nMismatches,
                                                  alignerScore, suboptimalScore, cigar, mdTag, xaTag, mateRefId, mateStartPos, templateLen))
            out.append(alignments)
        return out
