#!/bin/sh
# Regenerates tests/golden/tf_legacy from the bundles TensorFlow wrote for the reference's legacy model
# (data files, not source): the four index files, the first 66624 bytes (= the first 8 tensors: encoder layers
# 1 and 2, kernels + biases) of the features data file, and the rest of that file (encoder layers 3 to 6, 16 tensors) as
# verbatim byte ranges in files named after the offset they start at, each below 1 MiB: cut at tensor boundaries, the
# 1327104-byte kernel of layer 6 / conv2d_2 in two halves.  tests/trained_cases.py puts them back end to end.
# Run in the build container, where /root/reference exists.
set -e
L=/root/reference/.legacy/trained_weights/M4Depth-d6
D=$(dirname "$0")
DATA=$L/M4Depth/features/checkpoint-200000.data-00000-of-00001
cp $L/M4Depth/features/checkpoint-200000.index            $D/features.index
cp $L/M4Depth/features/optimizers/checkpoint-200000.index $D/features_optimizers.index
cp $L/M4Depth/upscaler/checkpoint-200000.index            $D/upscaler.index
cp $L/pipeline/checkpoint-200000.index                    $D/pipeline.index
head -c 66624 $DATA > $D/features.data-00000-of-00001
# offset size: layers 3-4 | layer 5 | layer 6 conv2d_1 and both biases | layer 6 conv2d_2 kernel, two halves
for range in "66624 775424" "842048 1033216" "1875264 886272" "2761536 663552" "3425088 663552"; do
    set -- $range
    tail -c +$(($1 + 1)) $DATA | head -c $2 > $D/$(printf 'features.data-00000-of-00001.at-%07d' $1)
done
chmod u+w $D/*.index $D/features.data-00000-of-00001*
