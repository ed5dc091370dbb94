// genbank.h -- GenBank query files: format detection, the reader and the annotated genes of every locus (host side).
// Restates what the ab-initio run uses of the reference's reader:
//   GBSplitter::determineFileType / findPositions / gotoEnd      reference src/genbank.cc:585-634, 661-759
//   GBFeature::GBFeature / checkRange / matches                   reference src/genbank.cc:370-540
//   GBProcessor::getAnnoSequence / getAnnoSequenceList / getSequence   reference src/genbank.cc:40-367
//   Gene::addUTR, sortGenePtrList, AnnoSequence::printGFF          reference src/gene.cc:1563-1656, 3155-3167, 2918-2930
#pragma once
#include <string>
#include <vector>
#include "genes.h"

namespace augx {

enum InputType { INPUT_UNKNOWN = 0, INPUT_GENBANK = 1, INPUT_FASTA = 2 }; // reference FileType, include/genbank.hh:27

// reference GBSplitter::determineFileType: GenBank when a line that begins with LOCUS is followed by one that begins with ORIGIN;
// else FASTA when no line but the headers holds anything but letters after a blank; else unknown (wrongChar: the offending character)
InputType detectInputType(const std::string &data, char *wrongChar = nullptr);

struct GbLocus {
    std::string name, seq;            // LOCUS name (first word, at most 99 characters); ORIGIN sequence, case kept
    long length = 0;                  // the `source` figure, or the number of bases when ORIGIN holds fewer
    std::vector<Transcript> genes;    // annotated transcripts sorted by begin (id "1", geneid = /gene= or NAME-k, source "database")
    std::vector<char> completeLeft, completeRight; // per transcript: no '<' / no '>' in the CDS (or, without CDS, the mRNA) feature
};

struct GbFile {
    std::vector<GbLocus> loci;
    std::string out, err;  // what the reference's reader writes to its output / error stream, in its order
};

struct GbOptions {
    bool utr = false;                       // --UTR on: mRNA features become UTR exons
    bool stopCodonExcludedFromCDS = false;  // the CDS features leave the stop codon out: it is added
    int verbosity = 3;                      // /genbank/verbosity
};

// Reads every locus of a GenBank text.  A locus the reference drops with a GBError is dropped with the reference's two lines on
// the error stream.  Returns false with `fatal` set to the reference's ProjectError message when nothing could be read.
bool readGenbank(const std::string &data, const GbOptions &go, GbFile &res, std::string &fatal);

// reference AnnoSequence::printGFF: "# Sequence NAME length=N" and the feature lines of every annotated transcript, source "database"
void printAnnotationGFF(std::string &out, const GbLocus &locus, const OutputOptions &o);

} // namespace augx
