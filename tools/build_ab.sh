#!/bin/bash
# Build an A/B variant of librmsf_hip.so into tools/_ab/librmsf_$1.so with extra -D flags ($2...).
set -e
name=$1; shift
make -C "$(dirname "$0")/../mdanalysis-mpi_amd/csrc" -j8 lib \
  OBJDIR=../../tools/_ab/$name OUT=../../tools/_ab/librmsf_$name.so EXTRA="$*"
rm -rf "$(dirname "$0")/_ab/$name"
