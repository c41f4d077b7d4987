"""Pre-aggregation of raw rows (reference analysis/pre_aggregation.py:19-61)."""
from pipelinedp_amd.data_extractors import DataExtractors


def preaggregate(col, backend, data_extractors: DataExtractors, partitions_sampling_prob: float = 1):
    """One element (partition_key, (count, sum, n_partitions, n_contributions))
    per (privacy_id, partition_key) of `col`: the count and sum of the values
    the privacy id contributed to the partition, the number of distinct
    partitions and the number of rows of the privacy id
    (AnalysisContributionBounder, analysis/contribution_bounders.py:37-77).
    A host convenience: UtilityAnalysisEngine.analyze does this reduction on
    the device when it is given raw rows."""
    if partitions_sampling_prob < 1:
        raise NotImplementedError("partitions_sampling_prob < 1 is not implemented")
    del backend  # the result is a list whatever the backend
    per_pid = {}
    for row in col:
        pid = data_extractors.privacy_id_extractor(row)
        pk = data_extractors.partition_extractor(row)
        value = data_extractors.value_extractor(row)
        per_pid.setdefault(pid, {}).setdefault(pk, []).append(value)
    out = []
    for partitions in per_pid.values():
        n_contributions = sum(len(values) for values in partitions.values())
        for pk, values in partitions.items():
            out.append((pk, (len(values), sum(values), len(partitions), n_contributions)))
    return out
