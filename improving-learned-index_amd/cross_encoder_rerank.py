"""CLI alias mirroring `python -m src.deep_impact.cross_encoder_rerank` (reference
cross_encoder_rerank.py:6-20)."""
from .cross_encoder_reranker import main

if __name__ == "__main__":
    main()
