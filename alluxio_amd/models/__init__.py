"""Workload-facing integrations (this framework has no neural models of its own: the "models"
it serves are training / inference input pipelines).  ``dataset`` gathers HBM-cached records
into device batches with one kernel launch per batch; ``fields`` parses batches of delimited text
into typed columns where they lie; ``json_fields`` does the same for batches of JSON Lines; ``parquet`` decodes the pages of Parquet
column chunks into the same columns and encodes such columns into the pages of a new Parquet file."""
from .dataset import (DeviceBatchLoader, FixedRecordDataset, IndexedRecordDataset, RaggedBatch,  # noqa: F401
                      build_delimited_index, read_index, write_index)
from .fields import (Column, FieldColumns, TextDictionary, extract_text, parse_fields,  # noqa: F401
                     read_delimited_columns, split_row)
from .json_fields import parse_json_fields, read_json_columns, unescape_json_text  # noqa: F401
from .parquet import (ParquetMetadata, ParquetStatistics, ParquetWriter, column_statistics,  # noqa: F401
                      parquet_matching_row_groups, parquet_metadata, parquet_page_table, parquet_row_groups,
                      read_parquet_columns, write_parquet_columns)
